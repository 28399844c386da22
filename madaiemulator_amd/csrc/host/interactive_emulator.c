/*
 * interactive_emulator -- command-line front end, drop-in for the reference's
 * src/interactive_emulator.c (same three modes, options, file formats and stdout protocol), and one mode more:
 *
 *   interactive_emulator estimate_thetas INPUT_MODEL_FILE MODEL_SNAPSHOT_FILE [OPTIONS]
 *   interactive_emulator interactive_mode MODEL_SNAPSHOT_FILE [OPTIONS]
 *   interactive_emulator print_thetas MODEL_SNAPSHOT_FILE
 *   interactive_emulator validate MODEL_SNAPSHOT_FILE [--pca_output] [--quiet]     (not in the reference)
 *   interactive_emulator validate MODEL_SNAPSHOT_FILE --holdout=FILE [--quiet]     (not in the reference)
 *   interactive_emulator validate MODEL_SNAPSHOT_FILE --folds=K | --groups=FILE [--pca_output] [--quiet]     (not in the reference)
 *
 * Kept quirks: --covariance_fn is atoi'd and compared with POWEREXPCOVFN=1 /
 * MATERN32=2 / MATERN52=3 (0 and 1 both mean power-exponential); --pca_variance falls through
 * into --pca_output and --quiet.
 *
 * interactive_mode is a request/response pipe (flush after every answer, :440 of the reference).
 * Points that are ALREADY waiting on stdin are answered as one GPU batch; a lone point is
 * answered immediately, so MCMC drivers that wait for each answer never dead-lock.  Reading/parsing,
 * the device and formatting/writing run as a three-stage pipeline (interactive_io.c); --binary selects
 * the reference's BINARY_INTERACTIVE_MODE framing (raw doubles in and out) at run time.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <getopt.h>
#include <unistd.h>
#include <assert.h>
#include <math.h>
#include <time.h>
#include "libemu.h"

struct cmdLineOpts {
	int regOrder, covFn, quietFlag, pcaOutputFlag, binaryFlag;
	double pca_variance;
	char *run_mode, *inputfile, *statefile, *holdoutfile, *groupsfile, *boxfile, *priorfile, *obsfile;
	double cutI, cutChi2;
	int level, gradientFlag;
	int best, bestGiven;
	int batch, batchGiven;           /* design --batch=K: K greedy picks (-1: not a number) */
	char *targetsfile;               /* design --targets=FILE: the gain over these points instead of the box */
	int targetsColumn, targetsColumnGiven;   /* ... whose parameters start at column K of every line (-1: not a number) */
	int walkers, steps, burn, thin, walkersGiven, burnGiven;
	unsigned long long seed;
	double stretch;
	int folds, foldsGiven, grid, uncertainty, pairs, surface, surfJ, surfK;
};

static const char useage[] =
	"useage:\n"
	"  interactive_emulator estimate_thetas INPUT_MODEL_FILE MODEL_SNAPSHOT_FILE [OPTIONS]\n"
	"or\n"
	"  interactive_emulator interactive_mode MODEL_SNAPSHOT_FILE [OPTIONS]\n"
	"or\n"
	"  interactive_emulator print_thetas MODEL_SNAPSHOT_FILE\n"
	"or\n"
	"  interactive_emulator validate MODEL_SNAPSHOT_FILE [--pca_output] [--quiet]  (leave-one-out mean and variance per training point)\n"
	"or\n"
	"  interactive_emulator validate MODEL_SNAPSHOT_FILE --holdout=FILE [--quiet]  (validation on a held-out campaign: FILE in the\n"
	"      INPUT_MODEL_FILE format; per point and PCA component mean, variance and decorrelated error, per component the\n"
	"      Mahalanobis distance and the joint log predictive density)\n"
	"or\n"
	"  interactive_emulator validate MODEL_SNAPSHOT_FILE --folds=K [--pca_output] [--quiet]  (K-fold cross-validation: training point i\n"
	"      is left out with fold i mod K, 2 <= K <= number of training points; mean and variance per training point from the\n"
	"      emulator on the other folds, per PCA component the Mahalanobis distance and joint log predictive density of the folds)\n"
	"or\n"
	"  interactive_emulator validate MODEL_SNAPSHOT_FILE --groups=FILE [--pca_output] [--quiet]  (leave-group-out: FILE holds one\n"
	"      integer per training point, the group it is left out with, 0 .. number of groups - 1, or -1 for never)\n"
	"  --holdout, --folds and --groups exclude each other.\n"
	"or\n"
	"  interactive_emulator sensitivity MODEL_SNAPSHOT_FILE [--box=FILE] [--grid=G] [--uncertainty] [--pairs] [--surface=j,k] [--prior=FILE] [--pca_output] [--quiet]  (main effects and Sobol\n"
	"      indices of the posterior mean, in closed form, for independent uniform inputs on a box: FILE holds one line \"lo hi\" per\n"
	"      parameter, default the range of the design.  Per output one line: variance, the first-order indices, the total\n"
	"      indices (NaN where the variance is 0); with --grid=G then, per output and parameter, the main-effect curve on G equally\n"
	"      spaced values, followed by the mean.  --uncertainty adds the emulator's own uncertainty: after the index lines, per output\n"
	"      one line with the posterior standard deviation of the mean, the box average of the posterior variance, the expected\n"
	"      variance and the expected first-order and total indices; with --grid, under every curve a line with its posterior\n"
	"      standard deviations.  --pairs appends, per output, one line with the second-order indices (V_jk - V_j - V_k) / V of the\n"
	"      pairs of parameters (0,1), (0,2), .., (d-2,d-1) (NaN where the variance is 0), and with --uncertainty then, per output, one\n"
	"      line with the expected interaction variances over the expected variance.  --surface=j,k with --grid=G appends, per output,\n"
	"      G lines of G values: the interaction effect of parameters j and k on the grid, row a at the a-th value of parameter j.\n"
	"      --prior=FILE in place of --box: one line per parameter, \"uniform LO HI\" or \"gaussian MEAN SD\" (SD > 0): the input measure\n"
	"      of each parameter, independent of the others; the curve and the surface of a Gaussian parameter run over MEAN -+ 2 SD.\n"
	"      Power-exponential covariance only)\n"
	"or\n"
	"  interactive_emulator implausibility MODEL_SNAPSHOT_FILE --observations=FILE [--cut=C] [--level=k] [--chi2=C2] [--gradient] [--quiet]  (points from\n"
	"      stdin to the end of input; one line per point whose k-th largest implausibility is <= C (default 3, k = 1) and whose joint\n"
	"      chi^2 is <= C2 (default: no cut): index, parameters, chi^2, log likelihood, the three largest implausibilities, the worst\n"
	"      output; with --gradient, behind them the d components of the log likelihood's gradient with respect to the parameters.\n"
	"      FILE: the number of outputs, one line \"value sd [rel]\" per output, optionally \"covariance\" and the matrix)\n"
	"or\n"
	"  interactive_emulator design MODEL_SNAPSHOT_FILE [--box=FILE | --prior=FILE] [--best=K] [--batch=K] [--targets=FILE [--targets-column=K]] [--pca_output] [--quiet]  (where to put the next model\n"
	"      run: candidate points from stdin to the end of input; one line per candidate: index, parameters, the expected drop of the\n"
	"      integrated posterior variance summed over the outputs if the model were run there, and that integrated variance as it\n"
	"      is now.  --best=K prints the K candidates with the largest drop, largest first, ties in input order.  --batch=K chooses a\n"
	"      batch of K runs greedily, each the largest drop GIVEN the picks before it, and prints them in pick order: index,\n"
	"      parameters, that conditional drop, and the integrated variance after the pick (K <= 256, at most 16384 candidates;\n"
	"      not with --best).  The measure as for\n"
	"      `sensitivity`.  Power-exponential covariance only.  --targets=FILE asks for the drop of the posterior variance over the\n"
	"      points of FILE instead -- one target per line, lines starting with # skipped, the d parameters from column K on (default 0),\n"
	"      further columns ignored, equal weights: the output of `sample` as it is, that of `implausibility` with --targets-column=1 --;\n"
	"      the lines then end with the expected drop of the targets' mean variance and that variance as it is now.  Any covariance\n"
	"      function; at most 65536 targets; not with --box, --prior or --batch)\n"
	"or\n"
	"  interactive_emulator sample MODEL_SNAPSHOT_FILE --observations=FILE [--box=FILE | --prior=FILE] [--walkers=W] [--steps=T] [--burn=B] [--thin=K] [--seed=S] [--stretch=a] [--quiet]\n"
	"      (posterior samples of the parameters given the observations of FILE (the format of `implausibility`), by the affine-invariant\n"
	"      ensemble sampler on the device.  The prior as the measure of `sensitivity`: --box, --prior, or uniform on the range of the\n"
	"      design.  W walkers (even, W / 2 >= d + 1; default max(64, 4 d)) start from draws of the prior and take T steps (default\n"
	"      1000); from step B on (default T / 4) every K-th step (default 1) is recorded.  stdout: one line per recorded sample, the d\n"
	"      parameters and the log posterior; stderr: the accepted fraction and per parameter mean, standard deviation, the 2.5 / 50 /\n"
	"      97.5 % quantiles and the integrated autocorrelation time.  --seed=S (default 1) picks the random numbers, --stretch=a > 1\n"
	"      (default 2) the scale of the stretch move)\n"
	"\n"
	"INPUT_MODEL_FILE can be \"-\" to read from standard input.\n"
	"\n"
	"Options which only influence estimate_thetas:\n"
	"  --regression_order=0..3   (const, linear, quadratic, cubic)\n"
	"  --covariance_fn=0|1 (POWER_EXPONENTIAL)  2 (MATERN32)  3 (MATERN52)\n"
	"  (-v FRAC) --pca_variance=FRAC : keep PCA components up to variance fraction FRAC\n"
	"options which influence interactive_mode:\n"
	"  (-q) --quiet: run without any extraneous output\n"
	"  (-z) --pca_output: emulator output is left in the pca space\n"
	"  --binary: points are read and results written as raw doubles (the reference's BINARY_INTERACTIVE_MODE build)\n"
	"  --observations=FILE: after a point's pairs its joint implausibility (chi^2), log likelihood and maximum implausibility\n"
	"      against the observations of FILE (the format of `implausibility`); not with --pca_output\n"
	"general options:\n"
	"  -h -? print this dialogue\n"
	"environment: GPEMU_DEVICE (HIP device), GPEMU_SEED, GPEMU_RESTARTS, GPEMU_JOBS, GPEMU_LOCKSTEP (restart threads\n"
	"sharing one device context, default 16), GPEMU_NTHREADS (with GPEMU_LOCKSTEP=1: threads with a context each)\n";

static int perr(const char *s) { fprintf(stderr, "%s\n", s); return EXIT_FAILURE; }

static double wall_s(void)
{
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* interactive_emulator.c:212-251 of the reference: "nt d N", N*d design values, N*nt outputs */
static int open_model_file(const char *name, gsl_matrix **xmodel_ptr, gsl_matrix **training_ptr)
{
	FILE *in = (!strcmp(name, "-") || !strcmp(name, "stdin")) ? stdin : fopen(name, "r");
	if (!in) return 0;
	int nt = 0, d = 0, n = 0;
	if (fscanf(in, "%d%*c", &nt) != 1 || fscanf(in, "%d%*c", &d) != 1 || fscanf(in, "%d%*c", &n) != 1) return 0;
	assert(nt > 0 && d > 0 && n > 0);
	gsl_matrix *x = gsl_matrix_alloc(n, d), *y = gsl_matrix_alloc(n, nt);
	for (int i = 0; i < n; i++) for (int j = 0; j < d; j++) if (fscanf(in, "%lf%*c", gsl_matrix_ptr(x, i, j)) != 1) return 0;
	for (int i = 0; i < n; i++) for (int j = 0; j < nt; j++) if (fscanf(in, "%lf%*c", gsl_matrix_ptr(y, i, j)) != 1) return 0;
	if (in != stdin) fclose(in);
	*xmodel_ptr = x; *training_ptr = y;
	return 1;
}

static int estimate_thetas(struct cmdLineOpts *o)
{
	gsl_matrix *xmodel = NULL, *training = NULL;
	double varfrac = 0.95;
	const double t_start = wall_s();
	/* one process per GPU (GPEMU_RANK / GPEMU_WORLD_SIZE, ranks.c): every rank trains its share and ends with the whole
	 * model; rank 0 alone writes MODEL_SNAPSHOT_FILE.  The ranks meet here, before anything else (ranks.c join_run). */
	gpemu_host_rank_device();
	gpemu_host_warm_start();                             /* the HIP runtime starts while the input file is being parsed */
	if (!open_model_file(o->inputfile, &xmodel, &training)) return perr("Input File read failed.");
	const double t_read = wall_s();
	FILE *out = fopen(gpemu_host_rank() == 0 ? o->statefile : "/dev/null", "w");
	if (!out) return perr("Opening statefile failed.");
	if (o->pca_variance <= 1.0 && o->pca_variance > 0) varfrac = o->pca_variance;
	if (o->covFn < 0 || o->covFn > 3) { fprintf(stderr, "#ERROR cov_fn_index %d not supported\n", o->covFn); exit(EXIT_FAILURE); }
	if (o->regOrder < 0 || o->regOrder > 3) { fprintf(stderr, "#ERROR regression_order %d not supported\n", o->regOrder); exit(EXIT_FAILURE); }
	multi_modelstruct *model = alloc_multimodelstruct(xmodel, training, o->covFn, o->regOrder, varfrac);
	if (!model) return perr("Failed to allocated multi_modelstruct.\n");
	const double t_alloc = wall_s();
	estimate_multi(model, out);
	fclose(out);
	const double t_train = wall_s();
	gpemu_host_ranks_finish();                       /* (ranks.c: the one gather is behind us) */
	if (gpemu_host_rank() == 0 && !getenv("GPEMU_NO_SNAPSHOT_CHECK")) {
		/* (not in the reference, which lets interactive_mode find out) */
		for (int i = 0; i < model->nr; i++)
			if (gpemu_host_emulator_setup_fails(model->pca_model_array[i]))
				fprintf(stderr, "# warning: component %d: the covariance matrix at the trained thetas (amplitude e^%.3f, nugget e^%.3f) is numerically "
				        "singular -- interactive_mode will refuse this snapshot (\"trying to cholesky a non postive def matrix\").  Training data without "
				        "noise drive the search, which is unbounded as in the reference, towards nugget -> 0; GPEMU_NUGGET_FLOOR=<log nugget>, e.g. -12, "
				        "gives the search a lower wall.\n", i,
				        gsl_vector_get(model->pca_model_array[i]->thetas, 0), gsl_vector_get(model->pca_model_array[i]->thetas, 1));
	}
	if (getenv("GPEMU_SEARCH_STATS"))
		fprintf(stderr, "# cli phases: rendezvous_read_input_s %.3f pca_alloc_s %.3f train_and_dump_s %.3f snapshot_check_s %.3f\n",
		        t_read - t_start, t_alloc - t_read, t_train - t_alloc, wall_s() - t_train);
	free_multimodelstruct(model);
	return EXIT_SUCCESS;
}

/* one batch of waiting points through every component's emulator (multivar_support.c:103-157, batched) */
struct emu_call { multi_emulator *emu; int pca_space, d; gpemu_observations *obs; };
struct obs_file { int nt, has_cov; double *z, *sd, *rel, *cov; };
static int read_observation_file(const char *name, int nt_model, struct obs_file *of);      /* below, with `implausibility` */

static void emu_points(void *user, int np, const double *pts, double *mean, double *var)
{
	struct emu_call *c = (struct emu_call *)user;
	gsl_matrix view = gpemu_matrix_view((double *)pts, (size_t)np, (size_t)c->d);
	emulate_points_multi(c->emu, &view, c->pca_space, mean, var);
}

/* --observations: joint implausibility (chi^2), log likelihood and maximum implausibility of the same batch, behind its pairs
 * (a second sweep of the batch: the calibration entry keeps its means and variances on the device) */
static void emu_points_extra(void *user, int np, const double *pts, double *extra)
{
	struct emu_call *c = (struct emu_call *)user;
	gsl_matrix view = gpemu_matrix_view((double *)pts, (size_t)np, (size_t)c->d);
	double *st = (double *)malloc(sizeof(double) * 5 * (size_t)np);
	emulate_points_multi_implausibility(c->emu, c->obs, &view, st, NULL);
	for (int q = 0; q < np; q++) {
		extra[(size_t)q * 3] = st[(size_t)q * 5];
		extra[(size_t)q * 3 + 1] = st[(size_t)q * 5 + 1];
		extra[(size_t)q * 3 + 2] = st[(size_t)q * 5 + 2];
	}
	free(st);
}

static int interactive_mode(struct cmdLineOpts *o)
{
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	const double t_start = wall_s();
	if (o->obsfile && o->pcaOutputFlag) return perr("--pca_output and --observations exclude each other: observations live in observable space");
	/* the HIP runtime starts while the snapshot is being parsed -- unless an observation file has to be judged first: it is
	 * parsed (against the snapshot's number of outputs) before any device is touched */
	if (!o->obsfile) gpemu_host_warm_start();
	/* nobody in this program reads emulator_struct.cinverse (the reference's interactive_mode does not either): spare every
	 * component the N x N download (512 MB at N = 8192) -- the library keeps filling it for callers that link libEmu */
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	struct obs_file of;
	if (o->obsfile) {
		if (!read_observation_file(o->obsfile, model->nt, &of)) return EXIT_FAILURE;
		gpemu_host_warm_start();
	}
	const double t_loaded = wall_s();
	multi_emulator *emu = alloc_multi_emulator(model);
	gpemu_observations *obs = o->obsfile ? alloc_observations(model, of.z, of.has_cov ? NULL : of.sd, of.has_cov ? of.cov : NULL, of.rel) : NULL;
	const double t_ready = wall_s();
	const int d = model->nparams, nt = model->nt;
	const int nout = o->pcaOutputFlag ? model->nr : nt;
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "%d\n", d);
		for (int i = 0; i < d; i++) fprintf(out, "%s%d\n", "param_", i);
		fprintf(out, "%d\n", 2 * nt + (obs ? 3 : 0));
		for (int i = 0; i < nt; i++) fprintf(out, "%s_%d\n%s_%d\n", "mean", i, "variance", i);
		if (obs) fprintf(out, "joint_implausibility\nlog_likelihood\nmax_implausibility\n");
	}
	fflush(out);
	/* the loop itself (interactive_emulator.c:414-441 of the reference): points already waiting on stdin are answered as
	 * one device batch, a lone point at once; reading/parsing, the device and formatting/writing overlap (interactive_io.c).
	 * The reference always prints nt pairs; in pca mode entries nr..nt-1 are whatever its vectors held: zeros here. */
	struct emu_call call = {emu, o->pcaOutputFlag, d, obs};
	struct gpemu_io_stats st;
	const int rc = obs ? gpemu_host_interactive_loop_extra(STDIN_FILENO, STDOUT_FILENO, d, nout, nt, o->binaryFlag, emu_points, 3, emu_points_extra,
	                                                       &call, &st)
	                   : gpemu_host_interactive_loop(STDIN_FILENO, STDOUT_FILENO, d, nout, nt, o->binaryFlag, emu_points, &call, &st);
	const char *want = getenv("GPEMU_IO_STATS");
	if (want && atoi(want) > 0)
		fprintf(stderr, "# interactive stats: points %ld batches %ld max_batch %d parse_s %.6f device_s %.6f format_s %.6f wall_s %.6f "
		        "load_snapshot_s %.6f alloc_multi_emulator_s %.6f components %d\n",
		        st.points, st.batches, st.max_batch, st.parse_seconds, st.compute_seconds, st.format_seconds, st.wall_seconds,
		        t_loaded - t_start, t_ready - t_loaded, model->nr);
	free_observations(obs);
	free_multi_emulator(emu);
	return rc == 0 ? 0 : EXIT_FAILURE;
}

static int validate_holdout(struct cmdLineOpts *o);      /* validate --holdout=FILE, below */
static int validate_lgo(struct cmdLineOpts *o);          /* validate --folds=K / --groups=FILE, below */

/* Leave-one-out validation of a trained snapshot (not in the reference, which leaves validation to a held-out campaign):
 * one line per training point in design order, "mean_0 variance_0 mean_1 variance_1 ..." -- what the emulator trained on
 * the other N - 1 points at the same thetas answers at that point (emulate_loo_multi) -- and one summary line per output
 * on stderr: the root mean square of (training value as given in the input - leave-one-out mean), so that in observable
 * space the PCA truncation shows, and the mean of residual^2 / variance, near 1 for a calibrated emulator. */
static int validate(struct cmdLineOpts *o)
{
	if (o->holdoutfile) return validate_holdout(o);
	if (o->foldsGiven || o->groupsfile) return validate_lgo(o);
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);               /* (as interactive_mode: nobody here reads emulator_struct.cinverse) */
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	multi_emulator *emu = alloc_multi_emulator(model);
	const int d = model->nparams, nt = model->nt, N = model->nmodel_points;
	const int nout = o->pcaOutputFlag ? model->nr : nt;
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "%d\n", d);
		for (int i = 0; i < d; i++) fprintf(out, "%s%d\n", "param_", i);
		fprintf(out, "%d\n", 2 * nt);
		for (int i = 0; i < nt; i++) fprintf(out, "%s_%d\n%s_%d\n", "mean", i, "variance", i);
	}
	double *mean = (double *)malloc(sizeof(double) * (size_t)N * nout), *var = (double *)malloc(sizeof(double) * (size_t)N * nout);
	emulate_loo_multi(emu, o->pcaOutputFlag, mean, var);
	for (int i = 0; i < N; i++) {
		for (int j = 0; j < nout; j++)
			fprintf(out, "%s%.17g %.17g", j ? " " : "", mean[(size_t)i * nout + j], var[(size_t)i * nout + j]);
		fprintf(out, "\n");
	}
	fflush(out);
	if (!o->quietFlag)
		for (int j = 0; j < nout; j++) {
			double ss = 0.0, sz = 0.0;
			for (int i = 0; i < N; i++) {
				const double given = o->pcaOutputFlag ? gsl_vector_get(model->pca_model_array[j]->training_vector, i)
				                                      : gsl_matrix_get(model->training_matrix, i, j);
				const double r = given - mean[(size_t)i * nout + j];
				ss += r * r;
				sz += r * r / var[(size_t)i * nout + j];
			}
			fprintf(stderr, "# loo output %d: rmse %.17g mean_standardised_sq %.17g\n", j, sqrt(ss / N), sz / N);
		}
	free(mean); free(var);
	free_multi_emulator(emu);
	return 0;
}

/* Validation of a trained snapshot on a held-out campaign (--holdout=FILE, FILE in the INPUT_MODEL_FILE format: "nt d N", the
 * N hold-out design points, their N x nt observed outputs).  The observations are projected onto the snapshot's PCA components
 * and every component is judged with the joint covariance between the hold-out points (emulate_points_multi_holdout), in PCA
 * space -- the only space these diagnostics exist in.  stdout: one line per hold-out point, "mean_0 variance_0 werr_0 mean_1
 * ..." over the components, werr the decorrelated error (independent N(0, 1) under the model; the per-point residual^2 /
 * variance of the leave-one-out mode ignores the correlations between the points).  stderr, per component: the squared
 * Mahalanobis distance (chi^2 with M degrees of freedom under the model), the joint log predictive density and the root
 * mean square of (projected observation - mean); then their totals. */
static int validate_holdout(struct cmdLineOpts *o)
{
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	gsl_matrix *xh = NULL, *yh = NULL;
	if (!open_model_file(o->holdoutfile, &xh, &yh)) return perr("Hold-out file read failed.");
	const int d = model->nparams, nt = model->nt, nr = model->nr;
	if ((int)xh->size2 != d || (int)yh->size2 != nt) {
		fprintf(stderr, "the hold-out file has %d parameters and %d outputs, the snapshot %d and %d\n", (int)xh->size2, (int)yh->size2, d, nt);
		return EXIT_FAILURE;
	}
	const size_t M = xh->size1;
	multi_emulator *emu = alloc_multi_emulator(model);
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "%d\n", d);
		for (int i = 0; i < d; i++) fprintf(out, "%s%d\n", "param_", i);
		fprintf(out, "%d\n", 3 * nr);
		for (int i = 0; i < nr; i++) fprintf(out, "%s_%d\n%s_%d\n%s_%d\n", "mean", i, "variance", i, "werr", i);
	}
	double *Y = (double *)malloc(sizeof(double) * M * (size_t)nt), *z = (double *)malloc(sizeof(double) * M * (size_t)nr);
	double *mean = (double *)malloc(sizeof(double) * M * (size_t)nr), *var = (double *)malloc(sizeof(double) * M * (size_t)nr);
	double *werr = (double *)malloc(sizeof(double) * M * (size_t)nr), *stat = (double *)malloc(sizeof(double) * 3 * (size_t)nr);
	double *maha = stat, *logdet = stat + nr, *logpdf = stat + 2 * nr, total = 0.0;
	for (size_t p = 0; p < M; p++) for (int t = 0; t < nt; t++) Y[p * nt + t] = gsl_matrix_get(yh, p, t);
	emulate_points_multi_holdout(emu, xh, Y, NULL, mean, var, werr, maha, logdet, logpdf, &total);
	for (size_t p = 0; p < M; p++) {
		for (int c = 0; c < nr; c++)
			fprintf(out, "%s%.17g %.17g %.17g", c ? " " : "", mean[p * nr + c], var[p * nr + c], werr[p * nr + c]);
		fprintf(out, "\n");
	}
	fflush(out);
	if (!o->quietFlag) {
		double dsum = 0.0;
		gpemu_host_project_observations(model, M, Y, z);
		for (int c = 0; c < nr; c++) {
			double ss = 0.0;
			for (size_t p = 0; p < M; p++) { const double r = z[(size_t)c * M + p] - mean[p * nr + c]; ss += r * r; }
			fprintf(stderr, "# holdout component %d: points %d mahalanobis %.17g log_density %.17g rmse %.17g\n", c, (int)M, maha[c], logpdf[c],
			        sqrt(ss / (double)M));
			dsum += maha[c];
		}
		fprintf(stderr, "# holdout total: components %d points %d mahalanobis %.17g log_density %.17g\n", nr, (int)M, dsum, total);
	}
	free(Y); free(z); free(mean); free(var); free(werr); free(stat);
	gsl_matrix_free(xh); gsl_matrix_free(yh);
	free_multi_emulator(emu);
	return 0;
}

/* K-fold (--folds=K: training point i in fold i mod K) and leave-group-out (--groups=FILE: one integer label per training
 * point, -1 = never left out) validation of a trained snapshot: every group is left out as a whole and predicted jointly by
 * the emulator on the other points at the same thetas (emulate_lgo_multi), so that replicated or clustered runs cannot carry
 * each other as they do in the leave-one-out mode.  stdout as in the leave-one-out mode (NaN for label -1).  stderr, per
 * output: rmse and mean residual^2 / variance over the points that were left out; per PCA component: the squared Mahalanobis
 * distances of the groups (chi^2 with dof = the number of left-out points under the model) and their joint log predictive
 * densities, both summed over the groups. */
static int validate_lgo(struct cmdLineOpts *o)
{
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int d = model->nparams, nt = model->nt, nr = model->nr, N = model->nmodel_points;
	const int nout = o->pcaOutputFlag ? nr : nt;
	int *group = (int *)malloc(sizeof(int) * (size_t)N), ngroups = 0, left = 0;
	if (o->groupsfile) {
		FILE *gf = fopen(o->groupsfile, "r");
		if (!gf) return perr("Error opening the groups file");
		for (int i = 0; i < N; i++) {
			if (fscanf(gf, "%d", &group[i]) != 1 || group[i] < -1) {
				fprintf(stderr, "the groups file needs %d integers >= -1, one per training point\n", N);
				return EXIT_FAILURE;
			}
			if (group[i] + 1 > ngroups) ngroups = group[i] + 1;
		}
		fclose(gf);
		if (ngroups < 1) return perr("the groups file leaves no point out");
	} else {
		if (o->folds < 2 || o->folds > N) {
			fprintf(stderr, "--folds=K needs 2 <= K <= %d training points\n", N);
			return EXIT_FAILURE;
		}
		ngroups = o->folds;
		for (int i = 0; i < N; i++) group[i] = i % ngroups;
	}
	for (int i = 0; i < N; i++) left += group[i] >= 0;
	multi_emulator *emu = alloc_multi_emulator(model);
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "%d\n", d);
		for (int i = 0; i < d; i++) fprintf(out, "%s%d\n", "param_", i);
		fprintf(out, "%d\n", 2 * nt);
		for (int i = 0; i < nt; i++) fprintf(out, "%s_%d\n%s_%d\n", "mean", i, "variance", i);
	}
	double *mean = (double *)malloc(sizeof(double) * (size_t)N * nout), *var = (double *)malloc(sizeof(double) * (size_t)N * nout);
	double *maha = (double *)malloc(sizeof(double) * (size_t)nr * ngroups), *logpdf = (double *)malloc(sizeof(double) * (size_t)nr * ngroups);
	emulate_lgo_multi(emu, o->pcaOutputFlag, ngroups, group, mean, var, maha, logpdf);
	for (int i = 0; i < N; i++) {
		for (int j = 0; j < nout; j++)
			fprintf(out, "%s%.17g %.17g", j ? " " : "", mean[(size_t)i * nout + j], var[(size_t)i * nout + j]);
		fprintf(out, "\n");
	}
	fflush(out);
	if (!o->quietFlag) {
		for (int j = 0; j < nout; j++) {
			double ss = 0.0, sz = 0.0;
			for (int i = 0; i < N; i++) {
				if (group[i] < 0) continue;
				const double given = o->pcaOutputFlag ? gsl_vector_get(model->pca_model_array[j]->training_vector, i)
				                                      : gsl_matrix_get(model->training_matrix, i, j);
				const double r = given - mean[(size_t)i * nout + j];
				ss += r * r;
				sz += r * r / var[(size_t)i * nout + j];
			}
			fprintf(stderr, "# lgo output %d: rmse %.17g mean_standardised_sq %.17g\n", j, sqrt(ss / left), sz / left);
		}
		for (int c = 0; c < nr; c++) {
			double ms = 0.0, ls = 0.0;
			for (int g = 0; g < ngroups; g++) { ms += maha[(size_t)c * ngroups + g]; ls += logpdf[(size_t)c * ngroups + g]; }
			fprintf(stderr, "# lgo component %d: maha %.17g dof %d logpdf %.17g\n", c, ms, left, ls);
		}
	}
	free(mean); free(var); free(maha); free(logpdf); free(group);
	free_multi_emulator(emu);
	return 0;
}

/* Sensitivity analysis of a trained snapshot (the reference's counterpart is the R code of src/libSA; here in closed form over a
 * box, emulate_sensitivity_multi): which parameter an output depends on, and how strongly.  stdout, per output, one line
 * "variance S_0 .. S_{d-1} T_0 .. T_{d-1}" -- S_j = V_j / V the first-order and T_j = VT_j / V the total-effect index, NaN where
 * V = 0 --; with --grid=G then, per output, d lines of G values each, E[output | x_j = lo_j + g (hi_j - lo_j) / (G - 1)] (G = 1:
 * the centre of the box), followed by a line holding E0.
 * --uncertainty (emulate_sensitivity_uncertainty_multi, emulate_main_effects_band_multi): after those lines, per output, one line
 * "sd(E0) IMSE E*[V] E*[V_0]/E*[V] .. E*[VT_0]/E*[V] .." -- the posterior standard deviation of the mean, the box average of the
 * posterior variance, the expected variance of the emulated function and its expected first-order and total parts over it --;
 * and with --grid=G every curve is followed by a line of G posterior standard deviations of its values.  Without the flag the
 * output is what it was before the flag existed.
 * --prior=FILE (emulate_sensitivity_measure_multi) in place of --box=FILE: per parameter "uniform LO HI" or "gaussian MEAN SD",
 * the input measure of that parameter.  lo / hi then hold MEAN / SD of a Gaussian parameter, as every emulate_sensitivity*
 * function reads them; glo / ghi are where its curve and surface run, MEAN -+ 2 SD (the box itself for a uniform parameter).
 * Without --prior every byte of output is what it was before the flag existed. */
/* a box or prior file that cannot be used, its message already written: status 1 by the layer's teardown-free exit (fatal.c).
 * A return from main would run exit()'s handlers, the HIP runtime's among them, beside the warm-start thread, which at this
 * point is usually still inside the runtime's start-up: the process then ends in abort() and not with status 1. */
static int bad_measure_file(void)
{
	gpemu_host_exit(EXIT_FAILURE);
	return EXIT_FAILURE;
}

/* the input measure of `sensitivity` and `design`: --prior=FILE, --box=FILE or the range of the design into lo, hi and kind (d each,
 * kind zeroed by the caller).  0, or the status to end with, its message already written. */
static int read_measure(const struct cmdLineOpts *o, const multi_modelstruct *model, double *lo, double *hi, int *kind)
{
	const int d = model->nparams, N = model->nmodel_points;
	if (o->boxfile && o->priorfile) { perr("--box=FILE and --prior=FILE exclude each other"); return bad_measure_file(); }
	if (o->priorfile) {
		FILE *pf = fopen(o->priorfile, "r");
		if (!pf) { perr("Error opening the prior file"); return bad_measure_file(); }
		for (int j = 0; j < d; j++) {
			char word[16];
			int ok = fscanf(pf, "%15s %lf %lf", word, &lo[j], &hi[j]) == 3 && isfinite(lo[j]) && isfinite(hi[j]);
			if (ok && !strcmp(word, "gaussian")) { kind[j] = 1 /* GPEMU_MEASURE_GAUSS */; ok = hi[j] > 0.0; }
			else if (ok) ok = !strcmp(word, "uniform") && hi[j] > lo[j];
			if (!ok) {
				fprintf(stderr, "the prior file needs %d lines \"uniform LO HI\" with LO < HI or \"gaussian MEAN SD\" with SD > 0, one per parameter\n", d);
				return bad_measure_file();
			}
		}
		fclose(pf);
	} else if (o->boxfile) {
		FILE *bf = fopen(o->boxfile, "r");
		if (!bf) { perr("Error opening the box file"); return bad_measure_file(); }
		for (int j = 0; j < d; j++)
			if (fscanf(bf, "%lf %lf", &lo[j], &hi[j]) != 2 || !(hi[j] > lo[j])) {
				fprintf(stderr, "the box file needs %d lines \"lo hi\" with lo < hi, one per parameter\n", d);
				return bad_measure_file();
			}
		fclose(bf);
	} else {
		for (int j = 0; j < d; j++) {
			lo[j] = hi[j] = gsl_matrix_get(model->xmodel, 0, j);
			for (int i = 1; i < N; i++) {
				const double x = gsl_matrix_get(model->xmodel, i, j);
				if (x < lo[j]) lo[j] = x;
				if (x > hi[j]) hi[j] = x;
			}
			if (!(hi[j] > lo[j])) {
				fprintf(stderr, "parameter %d does not vary over the design: give a box with --box=FILE\n", j);
				return EXIT_FAILURE;
			}
		}
	}
	return 0;
}

static int sensitivity(struct cmdLineOpts *o)
{
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);               /* (as interactive_mode: nobody here reads emulator_struct.cinverse) */
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int d = model->nparams, nt = model->nt, G = o->grid;
	const int nout = o->pcaOutputFlag ? model->nr : nt;
	if (model->cov_fn_index > 1) return perr("sensitivity: the closed form exists for the power-exponential covariance only");
	if (G < 0) return perr("--grid=G needs G >= 1");
	if ((o->pairs || o->surface) && d < 2) return perr("--pairs and --surface need a model with two parameters or more");
	if (o->surface && (G < 1 || o->surfJ == o->surfK || o->surfJ < 0 || o->surfK < 0 || o->surfJ >= d || o->surfK >= d))
		return perr("--surface=j,k needs two different parameters of 0 .. d - 1, and --grid=G");
	double *lo = (double *)malloc(sizeof(double) * (size_t)d), *hi = (double *)malloc(sizeof(double) * (size_t)d);
	int *kind = (int *)calloc((size_t)d, sizeof(int));                            /* GPEMU_MEASURE_UNIFORM */
	{
		const int rc = read_measure(o, model, lo, hi, kind);
		if (rc) return rc;
	}
	/* where the curves and the surface run */
	double *glo = (double *)malloc(sizeof(double) * (size_t)d), *ghi = (double *)malloc(sizeof(double) * (size_t)d);
	for (int j = 0; j < d; j++) {
		glo[j] = kind[j] ? lo[j] - 2.0 * hi[j] : lo[j];
		ghi[j] = kind[j] ? lo[j] + 2.0 * hi[j] : hi[j];
	}
	multi_emulator *emu = alloc_multi_emulator(model);
	if (o->priorfile) emulate_sensitivity_measure_multi(emu, kind);
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "%d\n", d);
		for (int j = 0; j < d; j++) {
			if (o->priorfile) fprintf(out, "%s%d %s %.17g %.17g\n", "param_", j, kind[j] ? "gaussian" : "uniform", lo[j], hi[j]);
			else fprintf(out, "%s%d %.17g %.17g\n", "param_", j, lo[j], hi[j]);
		}
		fprintf(out, "%d\n", nout);
	}
	double *e0 = (double *)malloc(sizeof(double) * (size_t)nout), *var = (double *)malloc(sizeof(double) * (size_t)nout);
	double *first = (double *)malloc(sizeof(double) * (size_t)nout * d), *total = (double *)malloc(sizeof(double) * (size_t)nout * d);
	emulate_sensitivity_multi(emu, o->pcaOutputFlag, lo, hi, e0, var, first, total);
	for (int t = 0; t < nout; t++) {
		fprintf(out, "%.17g", var[t]);
		for (int j = 0; j < d; j++) fprintf(out, " %.17g", var[t] != 0.0 ? first[(size_t)t * d + j] / var[t] : NAN);
		for (int j = 0; j < d; j++) fprintf(out, " %.17g", var[t] != 0.0 ? total[(size_t)t * d + j] / var[t] : NAN);
		fprintf(out, "\n");
	}
	if (o->uncertainty) {
		double *ve0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *imse = ve0 + nout, *evar = imse + nout;
		double *ef = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *et = ef + (size_t)nout * d;
		emulate_sensitivity_uncertainty_multi(emu, o->pcaOutputFlag, lo, hi, ve0, imse, evar, ef, et);
		for (int t = 0; t < nout; t++) {
			fprintf(out, "%.17g %.17g %.17g", sqrt(ve0[t] > 0.0 ? ve0[t] : 0.0), imse[t], evar[t]);
			for (int j = 0; j < d; j++) fprintf(out, " %.17g", evar[t] != 0.0 ? ef[(size_t)t * d + j] / evar[t] : NAN);
			for (int j = 0; j < d; j++) fprintf(out, " %.17g", evar[t] != 0.0 ? et[(size_t)t * d + j] / evar[t] : NAN);
			fprintf(out, "\n");
		}
		free(ve0); free(ef);
	}
	if (G > 0) {
		double *grid = (double *)malloc(sizeof(double) * (size_t)d * G), *mainv = (double *)malloc(sizeof(double) * (size_t)d * G * nout);
		double *sdv = o->uncertainty ? (double *)malloc(sizeof(double) * (size_t)d * G * nout) : NULL;
		for (int j = 0; j < d; j++)
			for (int g = 0; g < G; g++) grid[(size_t)j * G + g] = G > 1 ? glo[j] + g * (ghi[j] - glo[j]) / (G - 1) : 0.5 * (glo[j] + ghi[j]);
		if (sdv) emulate_main_effects_band_multi(emu, o->pcaOutputFlag, lo, hi, G, grid, e0, mainv, sdv);
		else emulate_main_effects_multi(emu, o->pcaOutputFlag, lo, hi, G, grid, e0, mainv);
		for (int t = 0; t < nout; t++) {
			for (int j = 0; j < d; j++) {
				for (int g = 0; g < G; g++) fprintf(out, "%s%.17g", g ? " " : "", mainv[((size_t)j * G + g) * nout + t]);
				fprintf(out, "\n");
				if (sdv) {
					for (int g = 0; g < G; g++) fprintf(out, "%s%.17g", g ? " " : "", sdv[((size_t)j * G + g) * nout + t]);
					fprintf(out, "\n");
				}
			}
			fprintf(out, "%.17g\n", e0[t]);
		}
		free(grid); free(mainv); free(sdv);
	}
	if (o->pairs) {
		/* per output one line of the d (d - 1) / 2 second-order indices; with --uncertainty then one line of E*[V_jk - V_j - V_k] / E*[V] */
		const size_t np = (size_t)d * (d - 1) / 2;
		double *vp = (double *)malloc(sizeof(double) * 2 * (size_t)nout * np), *in = vp + (size_t)nout * np;
		emulate_sensitivity_pairs_multi(emu, o->pcaOutputFlag, lo, hi, vp, in);
		for (int t = 0; t < nout; t++) {
			for (size_t p = 0; p < np; p++) fprintf(out, "%s%.17g", p ? " " : "", var[t] != 0.0 ? in[(size_t)t * np + p] / var[t] : NAN);
			fprintf(out, "\n");
		}
		if (o->uncertainty) {
			double *ve0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *imse = ve0 + nout, *evar = imse + nout;
			double *ef = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *et = ef + (size_t)nout * d;
			emulate_sensitivity_uncertainty_multi(emu, o->pcaOutputFlag, lo, hi, ve0, imse, evar, ef, et);
			emulate_sensitivity_pairs_uncertainty_multi(emu, o->pcaOutputFlag, lo, hi, vp, in);
			for (int t = 0; t < nout; t++) {
				for (size_t p = 0; p < np; p++) fprintf(out, "%s%.17g", p ? " " : "", evar[t] != 0.0 ? in[(size_t)t * np + p] / evar[t] : NAN);
				fprintf(out, "\n");
			}
			free(ve0); free(ef);
		}
		free(vp);
	}
	if (o->surface) {
		/* per output G lines of G values: the interaction effect of the pair on the grid of the curves */
		double *gj = (double *)malloc(sizeof(double) * 2 * (size_t)G), *gk = gj + G;
		double *jt = (double *)malloc(sizeof(double) * 2 * (size_t)G * G * nout), *it = jt + (size_t)G * G * nout;
		const int sj = o->surfJ, sk = o->surfK;
		for (int g = 0; g < G; g++) {
			gj[g] = G > 1 ? glo[sj] + g * (ghi[sj] - glo[sj]) / (G - 1) : 0.5 * (glo[sj] + ghi[sj]);
			gk[g] = G > 1 ? glo[sk] + g * (ghi[sk] - glo[sk]) / (G - 1) : 0.5 * (glo[sk] + ghi[sk]);
		}
		emulate_interaction_surface_multi(emu, o->pcaOutputFlag, lo, hi, sj, sk, G, gj, gk, e0, jt, it);
		for (int t = 0; t < nout; t++)
			for (int a = 0; a < G; a++) {
				for (int b = 0; b < G; b++) fprintf(out, "%s%.17g", b ? " " : "", it[((size_t)a * G + b) * nout + t]);
				fprintf(out, "\n");
			}
		free(gj); free(jt);
	}
	fflush(out);
	free(lo); free(hi); free(glo); free(ghi); free(kind); free(e0); free(var); free(first); free(total);
	free_multi_emulator(emu);
	return 0;
}

/* The observation file of `implausibility` (and of alloc_observations' callers): line 1 the number of outputs nt; then nt
 * lines "value sd [rel]" (sd > 0; rel >= 0, a relative model error, 0 where it is left out); then, optionally, a line
 * "covariance" and nt rows of nt numbers that replace sd^2.  Host logic only.  Returns 1, or 0 with the complaint on stderr. */
static int obs_complain(const char *what, int line)
{
	fprintf(stderr, "the observation file, line %d: %s\n(line 1: the number of outputs; then one line \"value sd [rel]\" per output, sd > 0, rel >= 0; "
	        "optionally a line \"covariance\" and one row of the covariance matrix per output)\n", line, what);
	return 0;
}

static int read_observation_file(const char *name, int nt_model, struct obs_file *of)
{
	FILE *f = fopen(name, "r");
	if (!f) { fprintf(stderr, "Error opening the observation file\n"); return 0; }
	char buf[65536], tail[8];
	int line = 1, nt = 0;
	memset(of, 0, sizeof *of);
	if (!fgets(buf, sizeof buf, f) || sscanf(buf, "%d %7s", &nt, tail) != 1 || nt < 1) { fclose(f); return obs_complain("the number of outputs is missing", line); }
	if (nt != nt_model) { fclose(f); fprintf(stderr, "the observation file has %d outputs, the model %d\n", nt, nt_model); return 0; }
	of->nt = nt;
	of->z = (double *)calloc((size_t)nt, sizeof(double)); of->sd = (double *)calloc((size_t)nt, sizeof(double));
	of->rel = (double *)calloc((size_t)nt, sizeof(double)); of->cov = (double *)calloc((size_t)nt * nt, sizeof(double));
	for (int t = 0; t < nt; t++) {
		line++;
		if (!fgets(buf, sizeof buf, f)) { fclose(f); return obs_complain("the file ends before every output has its line", line); }
		const int n = sscanf(buf, "%lf %lf %lf %7s", &of->z[t], &of->sd[t], &of->rel[t], tail);
		if (n != 2 && n != 3) { fclose(f); return obs_complain("two or three numbers are needed", line); }
		if (n == 2) of->rel[t] = 0.0;
		if (!isfinite(of->z[t]) || !isfinite(of->sd[t]) || !(of->sd[t] > 0.0) || !isfinite(of->rel[t]) || of->rel[t] < 0.0) {
			fclose(f);
			return obs_complain("a finite value, sd > 0 and rel >= 0 are needed", line);
		}
	}
	while (fgets(buf, sizeof buf, f)) {                   /* blank lines, then nothing or the covariance block */
		line++;
		char word[32];
		if (sscanf(buf, "%31s", word) != 1) continue;
		if (strcmp(word, "covariance") || of->has_cov) { fclose(f); return obs_complain("\"covariance\" or the end of the file is expected here", line); }
		of->has_cov = 1;
		for (int t = 0; t < nt; t++) {
			line++;
			if (!fgets(buf, sizeof buf, f)) { fclose(f); return obs_complain("the covariance matrix ends early", line); }
			char *p = buf, *end;
			for (int u = 0; u < nt; u++) {
				of->cov[(size_t)t * nt + u] = strtod(p, &end);
				if (end == p || !isfinite(of->cov[(size_t)t * nt + u])) { fclose(f); return obs_complain("a row of the covariance matrix needs one finite number per output", line); }
				p = end;
			}
			if (sscanf(p, "%7s", tail) == 1) { fclose(f); return obs_complain("a row of the covariance matrix has too many entries", line); }
		}
	}
	fclose(f);
	return 1;
}

/* History matching / calibration against observations (not in the reference's C; its R: libRbind/implausOverDesign.R): points
 * are read from stdin to the end of input, d numbers each; for every point with chi^2 <= --chi2 (default: no cut) and level-th
 * largest per-output implausibility <= --cut (defaults 3 and level 1: the customary 3 sigma cut on the maximum implausibility;
 * the reference's plots cut its SQUARED quantity at 1.8) one line "index p_0 .. p_{d-1} chi2 log_likelihood I1 I2 I3 worst" is
 * written.  The selection runs on the device; only the survivors come back.  stderr: the fraction kept, and c_perp with its
 * nt - r degrees of freedom, the misfit no parameter value can remove.  The observation file is parsed before any device is
 * touched. */
static int implausibility(struct cmdLineOpts *o)
{
	if (!o->obsfile) return perr("implausibility needs --observations=FILE");
	if (o->pcaOutputFlag) return perr("--pca_output and --observations exclude each other: observations live in observable space");
	if (o->level < 1 || o->level > 3 || o->cutI != o->cutI || o->cutChi2 != o->cutChi2) return perr("--level=k needs k in 1 .. 3, --cut and --chi2 a number or inf");
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	struct obs_file of;
	if (!read_observation_file(o->obsfile, model->nt, &of)) return EXIT_FAILURE;
	const int d = model->nparams;
	size_t cap = 1024, n = 0;
	double *v = (double *)malloc(sizeof(double) * cap), x;
	while (fscanf(stdin, "%lf", &x) == 1) {
		if (n == cap) v = (double *)realloc(v, sizeof(double) * (cap *= 2));
		v[n++] = x;
	}
	if (!feof(stdin) || n % (size_t)d) return perr("implausibility: stdin must hold whole points, d numbers each, and nothing else");
	const size_t np = n / (size_t)d;
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);               /* (as interactive_mode: nobody here reads emulator_struct.cinverse) */
	multi_emulator *emu = alloc_multi_emulator(model);
	gpemu_observations *obs = alloc_observations(model, of.z, of.has_cov ? NULL : of.sd, of.has_cov ? of.cov : NULL, of.rel);
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "# index");
		for (int j = 0; j < d; j++) fprintf(out, " param_%d", j);
		fprintf(out, " joint_implausibility log_likelihood max_implausibility second_implausibility third_implausibility worst_output");
		for (int j = 0; o->gradientFlag && j < d; j++) fprintf(out, " dlog_likelihood_dparam_%d", j);
		fprintf(out, "\n");
	}
	int nkeep = 0;
	if (np) {
		gsl_matrix pts = gpemu_matrix_view(v, np, (size_t)d);
		int *idx = (int *)malloc(sizeof(int) * np), *worst = (int *)malloc(sizeof(int) * np);
		double *st = (double *)malloc(sizeof(double) * 5 * np);
		emulate_points_multi_nonimplausible_worst(emu, obs, &pts, o->cutChi2, o->level, o->cutI, idx, st, worst, &nkeep);
		double *g = NULL;
		if (o->gradientFlag && nkeep) {
			/* --gradient: the survivors alone go through the two gradient sweeps */
			double *kv = (double *)malloc(sizeof(double) * (size_t)nkeep * d);
			for (int k = 0; k < nkeep; k++) memcpy(kv + (size_t)k * d, v + (size_t)idx[k] * d, sizeof(double) * d);
			gsl_matrix kept = gpemu_matrix_view(kv, (size_t)nkeep, (size_t)d);
			g = (double *)malloc(sizeof(double) * (size_t)nkeep * d);
			emulate_points_multi_logpdf_grad(emu, obs, &kept, NULL, g, NULL);
			free(kv);
		}
		for (int k = 0; k < nkeep; k++) {
			fprintf(out, "%d", idx[k]);
			for (int j = 0; j < d; j++) fprintf(out, " %.17g", v[(size_t)idx[k] * d + j]);
			fprintf(out, " %.17g %.17g %.17g %.17g %.17g %d", st[k * 5], st[k * 5 + 1], st[k * 5 + 2], st[k * 5 + 3], st[k * 5 + 4], worst[k]);
			for (int j = 0; g && j < d; j++) fprintf(out, " %.17g", g[(size_t)k * d + j]);
			fprintf(out, "\n");
		}
		free(idx); free(worst); free(st); free(g);
	}
	fflush(out);
	double c_perp; int dof;
	gpemu_host_observations_misfit(obs, &c_perp, &dof);
	fprintf(stderr, "# implausibility: kept %d of %zu points (fraction %.6g); c_perp %.17g with %d degrees of freedom\n", nkeep, np,
	        np ? (double)nkeep / (double)np : 0.0, c_perp, dof);
	free(v);
	free_observations(obs);
	free_multi_emulator(emu);
	return 0;
}

/* Where to put the next model run (emulate_design_gain_multi): candidates from stdin, d numbers each.  stdout, per candidate, one
 * line "index param_0 .. param_{d-1} gain imse": gain the expected drop of the integrated posterior variance, summed over the
 * outputs, if the model were run there (hyper-parameters as they are), imse that integrated variance as it is now (the same on
 * every line).  --best=K: the K candidates with the largest gain, largest first, ties in input order.  --batch=K: K greedy picks
 * (emulate_design_batch_multi) in pick order, "index param_0 .. gain imse_after": the drop by the pick given the picks before it and
 * the integrated variance once it is made.  --targets=FILE [--targets-column=K] (emulate_design_target_gain_multi): the same lines
 * with the drop of the equally weighted posterior variance over the points of FILE, summed over the outputs, and that variance as
 * it is now; FILE holds one target per line, lines starting with # are skipped, the d parameters start at column K (default 0). */
static const double *design_key;
static int design_order(const void *a, const void *b)
{
	const int i = *(const int *)a, j = *(const int *)b;
	if (design_key[i] != design_key[j]) return design_key[i] > design_key[j] ? -1 : 1;
	return i < j ? -1 : (i > j);
}

/* the targets of --targets=FILE: ns points of d numbers, from column `column` of every line that does not start with # */
static double *read_targets(const char *path, int d, int column, size_t *ns)
{
	FILE *tf = fopen(path, "r");
	if (!tf) { perr("design: cannot open the file of --targets"); return NULL; }
	size_t cap = 256, n = 0, len = 0;
	double *t = (double *)malloc(sizeof(double) * cap * (size_t)d);
	char *line = NULL;
	while (getline(&line, &len, tf) >= 0) {
		char *p = line + strspn(line, " \t\r\n");
		if (*p == '#' || !*p) continue;
		if (n == cap) t = (double *)realloc(t, sizeof(double) * (cap *= 2) * (size_t)d);
		int c = 0;
		for (; c < column + d; c++) {
			char *end;
			const double x = strtod(p, &end);
			if (end == p) break;
			if (c >= column) t[n * (size_t)d + (size_t)(c - column)] = x;
			p = end;
		}
		if (c < column + d) {
			fprintf(stderr, "design: target line %zu of %s has fewer than %d columns\n", n + 1, path, column + d);
			free(t); free(line); fclose(tf);
			return NULL;
		}
		n++;
	}
	free(line);
	fclose(tf);
	if (n < 1 || n > 65536) {
		perr("design: --targets=FILE needs 1 .. 65536 targets");
		free(t);
		return NULL;
	}
	*ns = n;
	return t;
}

static int design(struct cmdLineOpts *o)
{
	if (o->targetsfile && (o->boxfile || o->priorfile || o->batchGiven)) return perr("--targets=FILE excludes --box, --prior and --batch");
	if (o->targetsColumnGiven && !o->targetsfile) return perr("--targets-column=K needs --targets=FILE");
	if (o->targetsColumnGiven && o->targetsColumn < 0) return perr("--targets-column=K needs a number K >= 0");
	if (o->bestGiven && o->best < 1) return perr("--best=K needs K >= 1");
	if (o->batchGiven && o->bestGiven) return perr("--batch=K and --best=K exclude each other");
	if (o->batchGiven && (o->batch < 1 || o->batch > 256)) return perr("--batch=K needs a number 1 <= K <= 256");
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);               /* (as interactive_mode: nobody here reads emulator_struct.cinverse) */
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int d = model->nparams, nout = o->pcaOutputFlag ? model->nr : model->nt;
	if (model->cov_fn_index > 1 && !o->targetsfile)
		return perr("design: the closed form exists for the power-exponential covariance only (--targets=FILE takes every covariance function)");
	size_t cap = 1024, n = 0;
	double *v = (double *)malloc(sizeof(double) * cap), x;
	while (fscanf(stdin, "%lf", &x) == 1) {
		if (n == cap) v = (double *)realloc(v, sizeof(double) * (cap *= 2));
		v[n++] = x;
	}
	if (!feof(stdin) || n % (size_t)d) return perr("design: stdin must hold whole points, d numbers each, and nothing else");
	const size_t np = n / (size_t)d;
	if (o->batchGiven && ((size_t)o->batch > np || np > 16384))
		return perr("design: --batch=K needs at least K candidates and at most 16384");
	double *lo = (double *)malloc(sizeof(double) * (size_t)d), *hi = (double *)malloc(sizeof(double) * (size_t)d);
	int *kind = (int *)calloc((size_t)d, sizeof(int));                            /* GPEMU_MEASURE_UNIFORM */
	size_t ns = 0;
	double *targets = NULL;
	if (o->targetsfile) {
		targets = read_targets(o->targetsfile, d, o->targetsColumnGiven ? o->targetsColumn : 0, &ns);
		if (!targets) return EXIT_FAILURE;
	} else {
		const int rc = read_measure(o, model, lo, hi, kind);
		if (rc) return rc;
	}
	multi_emulator *emu = alloc_multi_emulator(model);
	if (o->priorfile) emulate_sensitivity_measure_multi(emu, kind);
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "# index");
		for (int j = 0; j < d; j++) fprintf(out, " param_%d", j);
		fprintf(out, o->batchGiven ? " conditional_imse_reduction imse_after\n" :
		             targets ? " expected_target_variance_reduction target_variance\n" : " expected_imse_reduction imse\n");
	}
	if (np && o->batchGiven) {
		double *ve0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *imse = ve0 + nout, *evar = imse + nout;
		double *ef = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *et = ef + (size_t)nout * d;
		emulate_sensitivity_uncertainty_multi(emu, o->pcaOutputFlag, lo, hi, ve0, imse, evar, ef, et);
		double now = 0.0;
		for (int t = 0; t < nout; t++) now += imse[t];
		int *pick = (int *)malloc(sizeof(int) * (size_t)o->batch);
		double *pg = (double *)malloc(sizeof(double) * (size_t)o->batch);
		emulate_design_batch_multi(emu, o->pcaOutputFlag, lo, hi, (int)np, v, o->batch, pick, pg);
		for (int k = 0; k < o->batch; k++) {
			now -= pg[k];
			fprintf(out, "%d", pick[k]);
			for (int j = 0; j < d; j++) fprintf(out, " %.17g", v[(size_t)pick[k] * d + j]);
			fprintf(out, " %.17g %.17g\n", pg[k], now);
		}
		free(ve0); free(ef); free(pick); free(pg);
	} else if (np) {
		double *ve0 = (double *)malloc(sizeof(double) * 3 * (size_t)nout), *imse = ve0 + nout, *evar = imse + nout;
		double *ef = (double *)malloc(sizeof(double) * 2 * (size_t)nout * d), *et = ef + (size_t)nout * d;
		double *gain = (double *)malloc(sizeof(double) * np * (size_t)nout), *total = (double *)malloc(sizeof(double) * np);
		if (targets) emulate_design_target_gain_multi(emu, o->pcaOutputFlag, (int)ns, targets, NULL, (int)np, v, gain, total, imse);
		else {
			emulate_sensitivity_uncertainty_multi(emu, o->pcaOutputFlag, lo, hi, ve0, imse, evar, ef, et);
			emulate_design_gain_multi(emu, o->pcaOutputFlag, lo, hi, (int)np, v, gain, total);
		}
		double now = 0.0;                                                          /* the integrated, or the targets', variance as it is */
		for (int t = 0; t < nout; t++) now += imse[t];
		int *idx = (int *)malloc(sizeof(int) * np);
		for (size_t q = 0; q < np; q++) idx[q] = (int)q;
		size_t nprint = np;
		if (o->bestGiven) {
			design_key = total;
			qsort(idx, np, sizeof(int), design_order);
			if ((size_t)o->best < np) nprint = (size_t)o->best;
		}
		for (size_t k = 0; k < nprint; k++) {
			fprintf(out, "%d", idx[k]);
			for (int j = 0; j < d; j++) fprintf(out, " %.17g", v[(size_t)idx[k] * d + j]);
			fprintf(out, " %.17g %.17g\n", total[idx[k]], now);
		}
		free(ve0); free(ef); free(gain); free(total); free(idx);
	}
	fflush(out);
	free(v); free(lo); free(hi); free(kind); free(targets);
	free_multi_emulator(emu);
	return 0;
}

static int print_thetas(struct cmdLineOpts *o)
{
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int nr = model->nr, d = model->nparams, N = model->nmodel_points;
	const int nthetas = (int)model->pca_model_array[0]->thetas->size;
	double vartot = 0;
	printf("#-- EMULATOR LENGTH SCALES (thetas) IN PCA SPACE -- #\n");
	for (int i = 0; i < nr; i++) vartot += gsl_vector_get(model->pca_evals_r, i);
	printf("#-- id\tpca-var\tScale\tNugget");
	for (int i = 0; i < d; i++) printf("\tlength_%d", i);
	printf(" -- #\n");
	for (int i = 0; i < nr; i++) {
		printf("%d\t", i);
		printf("%lf\t", gsl_vector_get(model->pca_evals_r, i) / vartot);
		for (int j = 0; j < nthetas; j++) printf("%lf\t", exp(gsl_vector_get(model->pca_model_array[i]->thetas, j)));
		printf("\n");
	}
	for (int i = 0; i < nr; i++) {
		char name[256];
		snprintf(name, sizeof name, "pca_emu_summary_%d.dat", i);
		fp = fopen(name, "w");
		if (!fp) continue;
		for (int j = 0; j < N; j++) {
			for (int k = 0; k < d; k++) fprintf(fp, "%lf\t", gsl_matrix_get(model->pca_model_array[i]->xmodel, j, k));
			fprintf(fp, "%lf\n", gsl_vector_get(model->pca_model_array[i]->training_vector, j));
		}
		fclose(fp);
	}
	return 0;
}

/* Posterior samples of the parameters given observations (emulate_sample_posterior_multi; the reference stops at the toy
 * Metropolis steps of r-fns/metropolis.R).  Every refusal is decided on the host before a device is touched.  stdout: one line per
 * recorded sample -- recorded step after recorded step, walker after walker --, the d parameters and the log posterior in %.17g.
 * stderr: the summary, and a warning where the recorded steps are fewer than 50 integrated autocorrelation times. */
static int sample(struct cmdLineOpts *o)
{
	if (!o->obsfile) return perr("sample needs --observations=FILE");
	if (o->pcaOutputFlag) return perr("--pca_output and --observations exclude each other: observations live in observable space");
	if (o->boxfile && o->priorfile) return perr("--box=FILE and --prior=FILE exclude each other");
	if (o->walkersGiven && (o->walkers < 2 || (o->walkers & 1))) return perr("--walkers=W needs an even W >= 2");
	if (!(o->stretch > 1.0) || !isfinite(o->stretch)) return perr("--stretch=a needs a finite a > 1");
	if (o->steps < 1 || o->thin < 1 || (o->burnGiven && o->burn < 0)) return perr("--steps=T needs T >= 1, --thin=K K >= 1, --burn=B B >= 0");
	FILE *fp = fopen(o->statefile, "r");
	if (!fp) return perr("Error opening file");
	multi_modelstruct *model = load_multi_modelstruct(fp);
	fclose(fp);
	const int d = model->nparams;
	const int W = o->walkersGiven ? o->walkers : (4 * d > 64 ? 4 * d : 64);
	if (W / 2 < d + 1) {
		fprintf(stderr, "--walkers=%d for %d parameters: each half of the walkers needs at least d + 1 of them, W >= %d\n", W, d, 2 * (d + 1));
		return EXIT_FAILURE;
	}
	struct obs_file of;
	if (!read_observation_file(o->obsfile, model->nt, &of)) return EXIT_FAILURE;
	double *lo = (double *)malloc(sizeof(double) * (size_t)d), *hi = (double *)malloc(sizeof(double) * (size_t)d);
	int *kind = (int *)calloc((size_t)d, sizeof(int));                            /* GPEMU_MEASURE_UNIFORM */
	{
		const int rc = read_measure(o, model, lo, hi, kind);
		if (rc) return rc;
	}
	gpemu_host_sample_args args = {W, o->steps, o->burnGiven ? o->burn : o->steps / 4, o->thin, o->seed, 0ull, o->stretch};
	const size_t nrec = (size_t)gpemu_host_sample_nrec(&args);
	gpemu_host_warm_start();
	setenv("GPEMU_SKIP_CINVERSE", "1", 0);               /* (as interactive_mode: nobody here reads emulator_struct.cinverse) */
	multi_emulator *emu = alloc_multi_emulator(model);
	gpemu_observations *obs = alloc_observations(model, of.z, of.has_cov ? NULL : of.sd, of.has_cov ? of.cov : NULL, of.rel);
	double *tx = (double *)malloc(sizeof(double) * (nrec * (size_t)W * d + 1)), *tl = (double *)malloc(sizeof(double) * (nrec * (size_t)W + 1));
	double *sm = (double *)malloc(sizeof(double) * 6 * (size_t)d), accept = 0.0;
	emulate_sample_posterior_multi(emu, obs, lo, hi, kind, &args, NULL, tx, tl, NULL, &accept, sm);
	FILE *out = stdout;
	if (!o->quietFlag) {
		fprintf(out, "#");
		for (int j = 0; j < d; j++) fprintf(out, " param_%d", j);
		fprintf(out, " log_posterior\n");
	}
	for (size_t r = 0; r < nrec * (size_t)W; r++) {
		for (int j = 0; j < d; j++) fprintf(out, "%.17g ", tx[r * d + j]);
		fprintf(out, "%.17g\n", tl[r]);
	}
	fflush(out);
	fprintf(stderr, "# sample: %d walkers, %d steps, %zu recorded (burn %d, thin %d), seed %llu, accepted fraction %.6g\n", W, args.nsteps, nrec,
	        args.burn, args.thin, args.seed, accept);
	for (int j = 0; j < d; j++) {
		fprintf(stderr, "# param_%d mean %.17g sd %.17g q2.5 %.17g q50 %.17g q97.5 %.17g tau %.6g\n", j, sm[j], sm[d + j], sm[2 * d + j],
		        sm[3 * d + j], sm[4 * d + j], sm[5 * d + j]);
		if (nrec && (double)nrec < 50.0 * sm[5 * d + j])
			fprintf(stderr, "# warning: param_%d: %zu recorded steps are fewer than 50 autocorrelation times (%.6g): run longer\n", j, nrec,
			        50.0 * sm[5 * d + j]);
	}
	free(tx); free(tl); free(sm); free(lo); free(hi); free(kind);
	free_observations(obs);
	free_multi_emulator(emu);
	return 0;
}

static struct cmdLineOpts *global_opt_parse(int argc, char **argv)
{
	static const char *optString = "r:c:v:zqh?";
	static const struct option longOpts[] = {
		{"regression_order", required_argument, NULL, 'r'}, {"covariance_fn", required_argument, NULL, 'c'},
		{"pca_variance", required_argument, NULL, 'v'},      {"pca_output", no_argument, NULL, 'z'},
		{"quiet", no_argument, NULL, 'q'},                    {"help", no_argument, NULL, 'h'},
		/* not in the reference: the corrected forms of gpemu.h (same as GPEMU_EXACT_GRAD=1 / GPEMU_MATERN_FIXED=1) */
		{"exact_gradient", no_argument, NULL, 1001},          {"matern_fixed", no_argument, NULL, 1002},
		/* the reference's compile-time BINARY_INTERACTIVE_MODE (interactive_emulator.c:119,392-396,418-438) as a run-time flag */
		{"binary", no_argument, NULL, 1003},
		/* validate on a held-out campaign instead of leave-one-out */
		{"holdout", required_argument, NULL, 1004},
		/* ... or by K folds / by groups read from a file, every group left out as a whole */
		{"folds", required_argument, NULL, 1005},             {"groups", required_argument, NULL, 1006},
		/* sensitivity: the box of the input measure, the number of main-effect values per parameter */
		{"box", required_argument, NULL, 1007},               {"grid", required_argument, NULL, 1008},
		/* ... and the emulator's own uncertainty about the indices and the curves */
		{"uncertainty", no_argument, NULL, 1009},
		/* ... second order: the indices of all pairs of parameters, the interaction effect of one pair on the grid */
		{"pairs", no_argument, NULL, 1010},                   {"surface", required_argument, NULL, 1011},
		/* ... under a measure per parameter, uniform or Gaussian, in place of the box */
		{"prior", required_argument, NULL, 1012},
		/* implausibility: the observation file, the cut on the level-th largest implausibility, the cut on the joint chi^2 */
		{"observations", required_argument, NULL, 1013},      {"cut", required_argument, NULL, 1014},
		{"level", required_argument, NULL, 1015},             {"chi2", required_argument, NULL, 1016},
		/* ... and the gradient of the log likelihood behind every printed line */
		{"gradient", no_argument, NULL, 1017},
		/* design: only the K candidates that gain most */
		{"best", required_argument, NULL, 1018},
		/* design: a greedy batch of K runs */
		{"batch", required_argument, NULL, 1025},
		/* design: the gain over the points of a file, whose parameters start at a column */
		{"targets", required_argument, NULL, 1026},           {"targets-column", required_argument, NULL, 1027},
		/* sample: the ensemble, the run and its random numbers */
		{"walkers", required_argument, NULL, 1019},           {"steps", required_argument, NULL, 1020},
		{"burn", required_argument, NULL, 1021},              {"thin", required_argument, NULL, 1022},
		{"seed", required_argument, NULL, 1023},              {"stretch", required_argument, NULL, 1024},
		{NULL, no_argument, NULL, 0}};
	struct cmdLineOpts *o = (struct cmdLineOpts *)calloc(1, sizeof *o);
	o->pca_variance = 0.99;
	o->cutI = 3.0; o->cutChi2 = INFINITY; o->level = 1;
	o->steps = 1000; o->thin = 1; o->seed = 1; o->stretch = 2.0;
	int idx, opt;
	while ((opt = getopt_long(argc, argv, optString, longOpts, &idx)) != -1) {
		switch (opt) {
		case 'r': o->regOrder = atoi(optarg); break;
		case 'c': o->covFn = atoi(optarg); break;
		case 'v':
			o->pca_variance = atof(optarg);
			if (o->pca_variance < 0.0 || o->pca_variance > 1.0) {
				fprintf(stderr, "# err pca_variance argument given incorrect value: %lf\n", o->pca_variance);
				o->pca_variance = 0.95;
				fprintf(stderr, "# using default value: %lf\n", o->pca_variance);
			}
			fprintf(stderr, "# var-frac: %lf\n", o->pca_variance);
			/* fall through (as the reference does) */
		case 'z': o->pcaOutputFlag = 1; /* fall through */
		case 'q': o->quietFlag = 1; break;
		case 1001: gpemu_host_set_modes(gpemu_host_modes() | 1 /* GPEMU_MODE_EXACT_GRAD */); break;
		case 1002: gpemu_host_set_modes(gpemu_host_modes() | 2 /* GPEMU_MODE_MATERN_LOG */); break;
		case 1003: o->binaryFlag = 1; break;
		case 1004: o->holdoutfile = optarg; break;
		case 1005: o->folds = atoi(optarg); o->foldsGiven = 1; break;
		case 1006: o->groupsfile = optarg; break;
		case 1007: o->boxfile = optarg; break;
		case 1008: o->grid = atoi(optarg); if (o->grid < 1) o->grid = -1; break;
		case 1009: o->uncertainty = 1; break;
		case 1010: o->pairs = 1; break;
		case 1011:
			o->surface = 1;
			if (sscanf(optarg, "%d,%d", &o->surfJ, &o->surfK) != 2) o->surfJ = o->surfK = -1;
			break;
		case 1012: o->priorfile = optarg; break;
		case 1013: o->obsfile = optarg; break;
		case 1014: o->cutI = !strcmp(optarg, "inf") ? INFINITY : atof(optarg); break;
		case 1015: o->level = atoi(optarg); break;
		case 1016: o->cutChi2 = !strcmp(optarg, "inf") ? INFINITY : atof(optarg); break;
		case 1017: o->gradientFlag = 1; break;
		case 1018: o->best = atoi(optarg); o->bestGiven = 1; break;
		case 1019: o->walkers = atoi(optarg); o->walkersGiven = 1; break;
		case 1020: o->steps = atoi(optarg); break;
		case 1021: o->burn = atoi(optarg); o->burnGiven = 1; break;
		case 1022: o->thin = atoi(optarg); break;
		case 1023: o->seed = strtoull(optarg, NULL, 0); break;
		case 1024: o->stretch = atof(optarg); break;
		case 1025: {
			char *end;
			const long k = strtol(optarg, &end, 10);
			o->batch = (*optarg && !*end && k >= 1 && k <= 256) ? (int)k : -1;
			o->batchGiven = 1;
			break;
		}
		case 1026: o->targetsfile = optarg; break;
		case 1027: {
			char *end;
			const long k = strtol(optarg, &end, 10);
			o->targetsColumn = (*optarg && !*end && k >= 0 && k <= 1 << 20) ? (int)k : -1;
			o->targetsColumnGiven = 1;
			break;
		}
		case 'h':
		case '?': exit(perr(useage));
		default: break;
		}
	}
	if (optind >= argc) exit(perr(useage));
	if ((o->holdoutfile != NULL) + o->foldsGiven + (o->groupsfile != NULL) > 1) exit(perr(useage));
	o->run_mode = argv[optind];
	if (o->gradientFlag && (strcmp(o->run_mode, "implausibility") || o->binaryFlag))
		exit(perr("--gradient belongs to `implausibility` and prints text: not with another mode, not with --binary"));
	if (!strcmp(o->run_mode, "estimate_thetas")) {
		if (optind + 2 >= argc) exit(perr(useage));
		o->inputfile = argv[optind + 1];
		o->statefile = argv[optind + 2];
	} else {
		if (optind + 1 >= argc) exit(perr(useage));
		o->statefile = argv[optind + 1];
	}
	return o;
}

int main(int argc, char **argv)
{
	if (argc < 3) return perr(useage);
	const char *dev = getenv("GPEMU_DEVICE");
	if (dev) gpemu_host_set_device(atoi(dev));
	struct cmdLineOpts *o = global_opt_parse(argc, argv);
	int rc;
	if (!strcmp(o->run_mode, "estimate_thetas")) rc = estimate_thetas(o);
	else if (!strcmp(o->run_mode, "interactive_mode")) rc = interactive_mode(o);
	else if (!strcmp(o->run_mode, "print_thetas")) rc = print_thetas(o);
	else if (!strcmp(o->run_mode, "validate")) rc = validate(o);
	else if (!strcmp(o->run_mode, "sensitivity")) rc = sensitivity(o);
	else if (!strcmp(o->run_mode, "implausibility")) rc = implausibility(o);
	else if (!strcmp(o->run_mode, "design")) rc = design(o);
	else if (!strcmp(o->run_mode, "sample")) rc = sample(o);
	else { free(o); return perr(useage); }
	free(o);
	return rc;
}
