/*
 * libemu.h -- host-side (C99) mirror of the reference's libEmu / emulator
 * interface for the GP hot path, implemented on the MI355X device library
 * (include/gpemu.h).  Same names, argument meaning and error behaviour as the
 * reference headers, one header instead of eleven:
 *
 *   optstruct.h:25-88        struct optstruct            (field order kept)
 *   modelstruct.h:28-98      struct modelstruct          (field order kept)
 *   emulator_struct.h:20-29  struct emulator_struct      (field order kept)
 *   multi_modelstruct.h:18-61, multivar_support.h:11-20
 *   libEmu/estimate_threaded.h:18-29  struct estimate_thetas_params
 *   libEmu/{emulator,regression,estimator-fns,maxmultimin,emulate-fns}.h prototypes
 *
 * What differs from the reference, by design:
 *   - every O(N^2)/O(N^3) operation runs on the GPU; there is no CPU path for them;
 *   - log det C is 2*sum(log L_ii) instead of log((prod L_ii)^2) (the product under/overflows);
 *   - evalFnGradMulti shares ONE factorisation between value and gradient;
 *   - emulate_points() is added: a batch of query points per call.
 */
#ifndef GPEMU_LIBEMU_H
#define GPEMU_LIBEMU_H

#include <stdio.h>
#include <pthread.h>
#include "gsl_compat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define POWEREXPCOVFN 1
#define MATERN32 2
#define MATERN52 3

struct modelstruct;

typedef struct optstruct {
	int nthetas;
	int nparams;
	int nmodel_points;
	int nemulate_points;
	int regression_order;
	int nregression_fns;
	int fixed_nugget_mode;
	double fixed_nugget;
	int cov_fn_index;
	int use_data_scales;
	gsl_matrix *grad_ranges;          /* nthetas x 2 search box */
} optstruct;

typedef struct modelstruct {
	gsl_matrix *xmodel;               /* nmodel_points x nparams */
	gsl_vector *training_vector;      /* nmodel_points */
	gsl_vector *thetas;               /* nthetas */
	gsl_vector *sample_scales;        /* nparams */
	struct optstruct *options;
	void (*makeHVector)(gsl_vector *h_vector, gsl_vector *x_location, int nparams);
	double (*covariance_fn)(gsl_vector *, gsl_vector *, gsl_vector *, int, int);
	void (*makeGradMatLength)(gsl_matrix *dCdTheta, gsl_matrix *xmodel, double thetaLength, int index,
	                          int nmodel_points, int nparams);
} modelstruct;

typedef struct emulator_struct {
	int nparams;
	int nmodel_points;
	int nregression_fns;
	int nthetas;
	struct modelstruct *model;
	gsl_matrix *cinverse;
	gsl_vector *beta_vector;
	gsl_matrix *h_matrix;
} emulator_struct;

typedef struct multi_modelstruct {
	int nt;
	int nr;
	int nparams;
	int nmodel_points;
	int cov_fn_index;
	int regression_order;
	gsl_matrix *xmodel;
	gsl_matrix *training_matrix;
	gsl_vector *training_mean;
	modelstruct **pca_model_array;
	gsl_vector *pca_evals_r;
	gsl_matrix *pca_evecs_r;
	gsl_matrix *pca_zmatrix;
} multi_modelstruct;

typedef struct multi_emulator {
	int nt;
	int nr;
	int nparams;
	int nmodel_points;
	int nregression_fns;
	int nthetas;
	multi_modelstruct *model;
	emulator_struct **emu_struct_array;
} multi_emulator;

struct estimate_thetas_params {
	struct optstruct *options;
	struct modelstruct *the_model;
	gsl_rng *random_number;
	gsl_matrix *h_matrix;
	int max_tries;
	int success_count;
	double lhood_current;
	double my_best;
};

/* ---- libEmu/emulator.h ------------------------------------------------- */
double covariance_fn_gaussian(gsl_vector *xm, gsl_vector *xn, gsl_vector *thetas, int nthetas, int nparams);
double covariance_fn_matern_three(gsl_vector *xm, gsl_vector *xn, gsl_vector *thetas, int nthetas, int nparams);
double covariance_fn_matern_five(gsl_vector *xm, gsl_vector *xn, gsl_vector *thetas, int nthetas, int nparams);
void derivative_l_gauss(gsl_matrix *dCdTheta, gsl_matrix *xmodel, double thetaLength, int index, int nmodel_points, int nparams);
void derivative_l_matern_three(gsl_matrix *dCdTheta, gsl_matrix *xmodel, double thetaLength, int index, int nmodel_points, int nparams);
void derivative_l_matern_five(gsl_matrix *dCdTheta, gsl_matrix *xmodel, double thetaLength, int index, int nmodel_points, int nparams);
void makeCovMatrix_fnptr(gsl_matrix *cov_matrix, gsl_matrix *xmodel, gsl_vector *thetas, int nmodel_points, int nthetas,
                         int nparams, double (*covariance_fn_ptr)(gsl_vector *, gsl_vector *, gsl_vector *, int, int));
void makeKVector_fnptr(gsl_vector *kvector, gsl_matrix *xmodel, gsl_vector *xnew, gsl_vector *thetas, int nmodel_points,
                       int nthetas, int nparams,
                       double (*covariance_fn_ptr)(gsl_vector *, gsl_vector *, gsl_vector *, int, int));

/* the process-wide pointers of the reference's headers and the entry points that use them (set by set_global_ptrs) */
extern double (*covariance_fn)(gsl_vector *, gsl_vector *, gsl_vector *, int, int);
extern void (*makeHVector)(gsl_vector *h_vector, gsl_vector *x_location, int nparams);
extern void (*makeGradMatLength)(gsl_matrix *dCdTheta, gsl_matrix *xmodel, double thetaLength, int index, int nmodel_points,
                                 int nparams);
void makeCovMatrix(gsl_matrix *cov_matrix, gsl_matrix *xmodel, gsl_vector *thetas, int nmodel_points, int nthetas, int nparams);
void makeKVector(gsl_vector *kvector, gsl_matrix *xmodel, gsl_vector *xnew, gsl_vector *thetas, int nmodel_points, int nthetas,
                 int nparams);
void makeHMatrix(gsl_matrix *h_matrix, gsl_matrix *xmodel, int nmodel_points, int nparams, int nregression_fns);

void print_matrix(gsl_matrix *m, int nx, int ny);
void initialise_new_x(gsl_matrix *new_x, int nparams, int nemulate_points, double emulate_min, double emulate_max);

/* ---- libEmu/regression.h ------------------------------------------------ */
void makeHVector_trivial(gsl_vector *h_vector, gsl_vector *x_location, int nparams);
void makeHVector_linear(gsl_vector *h_vector, gsl_vector *x_location, int nparams);
void makeHVector_quadratic(gsl_vector *h_vector, gsl_vector *x_location, int nparams);
void makeHVector_cubic(gsl_vector *h_vector, gsl_vector *x_location, int nparams);
void makeHMatrix_fnptr(gsl_matrix *h_matrix, gsl_matrix *xmodel, int nmodel_points, int nparams, int nregression_fns,
                       void (*makeHVector_ptr)(gsl_vector *, gsl_vector *, int));

/* ---- host-matrix interface below evalFnMulti / emulate_point (what libRbind calls; lowlevel.c) ------------- */
void chol_inverse_cov_matrix(optstruct *options, gsl_matrix *temp_matrix, gsl_matrix *result_matrix, double *final_determinant_c);
void estimateBeta(gsl_vector *beta_vector, gsl_matrix *h_matrix, gsl_matrix *cinverse, gsl_vector *trainingvector,
                  int nmodel_points, int nregression_fns);
double estimateSigma(gsl_matrix *cinverse, void *params_in);
double getLogLikelyhood(gsl_matrix *cinverse, double det_cmatrix, gsl_matrix *xmodel, gsl_vector *trainingvector,
                        gsl_vector *thetas, gsl_matrix *h_matrix, int nmodel_points, int nthetas, int nparams,
                        int nregression_fns, void (*makeHVector)(gsl_vector *, gsl_vector *, int));
double makeEmulatedMean(gsl_matrix *inverse_cov_matrix, gsl_vector *training_vector, gsl_vector *kplus_vector,
                        gsl_vector *h_vector, gsl_matrix *h_matrix, gsl_vector *beta_vector, int nmodel_points);
double makeEmulatedVariance(gsl_matrix *inverse_cov_matrix, gsl_vector *kplus_vector, gsl_vector *h_vector,
                            gsl_matrix *h_matrix, double kappa, int nmodel_points, int nregression_fns);
double getGradientCn(gsl_matrix *dCdtheta, gsl_matrix *cinverse, gsl_vector *training_vector, int nmodel_points, int nthetas);

/* ---- libEmu/maxmultimin.h ------------------------------------------------ */
double evalFnMulti(const gsl_vector *theta_vec_less_amp, void *params_in);
/* extension: evalFnMulti for every row of a matrix (the first nthetas-1 entries of each row are read), factored in
 * lock-step batches on the device */
void evalFnMultiList(const gsl_matrix *theta_rows_less_amp, void *params_in, double *answer);
void gradFnMulti(const gsl_vector *theta_vec_less_amp, void *params_in, gsl_vector *grad_vec);
void evalFnGradMulti(const gsl_vector *theta_vec, void *params, double *fnval, gsl_vector *grad_vec);
double estimateSigmaFull(gsl_vector *thetas_less_amp, void *params_in);
void maxWithMultiMin(struct estimate_thetas_params *params);
int doOptimizeMultiMin(double (*fn)(const gsl_vector *, void *),
                       void (*gradientFn)(const gsl_vector *, void *, gsl_vector *),
                       void (*fnGradFn)(const gsl_vector *, void *, double *, gsl_vector *),
                       gsl_vector *thetaInit, gsl_vector *thetaFinal, void *args);
void set_random_init_value(gsl_rng *rand, gsl_vector *x, gsl_matrix *ranges, int nthetas);

/* ---- libEmu/estimate_threaded.h ------------------------------------------ */
void estimate_thetas_threaded(modelstruct *the_model, optstruct *options);
int get_number_cpus(void);
void setup_params(struct estimate_thetas_params *params_array, modelstruct *the_model, optstruct *options, int nthreads, int max_tries);
void *estimate_thread_function(void *args);
void fprintPt(FILE *f, pthread_t pt);

/* ---- resultstruct.h:20-36 + libEmu/emulate-fns.h:13-27 (legacy_api.c) ------- */
typedef struct resultstruct {
	gsl_matrix *new_x;                /* nemulate_points x nparams */
	gsl_vector *emulated_mean;
	gsl_vector *emulated_var;
	optstruct *options;
	modelstruct *model;
} resultstruct;
void alloc_resultstruct(resultstruct *res, optstruct *opts);
void free_resultstruct(resultstruct *res);
void copy_resultstruct(resultstruct *dst, resultstruct *src);
void fill_resultstruct(resultstruct *res, optstruct *options, char **input_data);
void emulate_model_results(modelstruct *the_model, optstruct *options, resultstruct *results);
void emulateAtPoint(modelstruct *the_model, gsl_vector *the_point, optstruct *options, double *the_mean, double *the_variance);
void emulateAtPointList(modelstruct *the_model, gsl_matrix *point_list, optstruct *options, double *the_mean, double *the_variance);
void emulateQuick(modelstruct *the_model, gsl_vector *the_point, optstruct *options, double *mean_out, double *var_out,
                  gsl_matrix *h_matrix, gsl_matrix *cinverse, gsl_vector *beta_vector);
void emulate_ith_location(modelstruct *the_model, optstruct *options, resultstruct *results, int i, gsl_matrix *h_matrix,
                          gsl_matrix *cinverse, gsl_vector *beta_vector);

/* ---- modelstruct.h / optstruct.h ------------------------------------------ */
/* the older, optstruct-sized forms and the optstruct helpers (legacy_api.c; callers: libRbind, estimate_threaded.c:57-68) */
void alloc_modelstruct(modelstruct *the_model, optstruct *options);
void free_modelstruct(modelstruct *the_model);
void copy_modelstruct(modelstruct *dst, modelstruct *src);
void fill_modelstruct(modelstruct *the_model, optstruct *options, char **input_data);
void dump_modelstruct(FILE *fptr, modelstruct *the_model, optstruct *opts);
void load_modelstruct(FILE *fptr, modelstruct *the_model, optstruct *opts);
void free_optstruct(optstruct *opts);
void copy_optstruct(optstruct *dst, optstruct *src);
void dump_optstruct(FILE *fptr, optstruct *opts);
void load_optstruct(FILE *fptr, optstruct *opts);
void setup_cov_fn(optstruct *opts);
void setup_regression(optstruct *opts);
modelstruct *alloc_modelstruct_2(gsl_matrix *xmodel, gsl_vector *training_vector, int cov_fn_index, int regression_order);
void free_modelstruct_2(modelstruct *model);
void dump_modelstruct_2(FILE *fptr, modelstruct *the_model);
modelstruct *load_modelstruct_2(FILE *fptr);
void set_global_ptrs(modelstruct *model);
gsl_vector *fill_sample_scales_vec(gsl_matrix *xmodel);
void setup_optimization_ranges(optstruct *options, modelstruct *the_model);

/* ---- emulator_struct.h ------------------------------------------------------ */
emulator_struct *alloc_emulator_struct(modelstruct *model);
void free_emulator_struct(emulator_struct *e);
void emulate_point(emulator_struct *e, gsl_vector *point, double *mean, double *variance);
void makeHMatrix_es(gsl_matrix *h_matrix, emulator_struct *e);
void makeCovMatrix_es(gsl_matrix *cov_matrix, emulator_struct *e);
void makeKVector_es(gsl_vector *kvector, gsl_vector *point, emulator_struct *e);
void estimateBeta_es(gsl_vector *beta_vector, emulator_struct *e);
/* alloc_emulator_struct with the say on the host copy of C^-1 (a public field, N x N doubles downloaded and mirrored:
 * most of the call's time at large N): 0 leaves e->cinverse allocated but unfilled for callers that never read it */
emulator_struct *gpemu_host_alloc_emulator(modelstruct *model, int fill_cinverse);
/* ... for the n components of a multi-output model at once: one lock-step factorisation (gpemu_predict_setup_batch) */
void gpemu_host_alloc_emulators(modelstruct **models, int n, int fill_cinverse, emulator_struct **out);
/* the process's one-off device start-up costs on a thread of its own while the caller reads its input (device_bridge.c) */
void gpemu_host_warm_start(void);
void gpemu_host_warm_wait(void);
/* extension: npoints query rows (npoints x nparams), mean/variance arrays of npoints */
void emulate_points(emulator_struct *e, gsl_matrix *points, double *mean, double *variance);
/* emulate_points in two halves (device work runs in between): used to query all PCA components at the same time */
void emulate_points_enqueue(emulator_struct *e, gsl_matrix *points);
void emulate_points_collect(emulator_struct *e, int npoints, double *mean, double *variance);
/* the posterior mean alone (makeEmulatedMean, emulator.c:672-704): the device's fused k-vector . gamma sweep, no variance,
 * no N^2 product; agrees with emulate_points' mean to rounding (another summation order).  Errors end in gpemu_host_fatal. */
void emulate_points_mean(emulator_struct *e, gsl_matrix *points, double *mean);
void emulate_points_mean_enqueue(emulator_struct *e, gsl_matrix *points);
void emulate_points_mean_collect(emulator_struct *e, int npoints, double *mean);
/* the posterior mean and its gradient with respect to the query point (gpemu_predict_mean_grad in gpemu.h): grad is
 * npoints x nparams row-major, mean may be NULL.  Errors end in gpemu_host_fatal, as emulate_points_mean's do. */
void emulate_points_mean_grad(emulator_struct *e, gsl_matrix *points, double *mean, double *grad);
void emulate_points_mean_grad_enqueue(emulator_struct *e, gsl_matrix *points);
void emulate_points_mean_grad_collect(emulator_struct *e, int npoints, double *mean, double *grad);
/* mean, variance and the gradients of both with respect to the query point: grad_mean and grad_variance are npoints x
 * nparams row-major.  Any output may be NULL, but not all of them.  mean, variance and grad_variance come from
 * gpemu_predict_var_grad (gpemu.h: two N^2 products, the batch buffers of emulate_points, and on the first call a transposed
 * copy of L^-1 of 8 N (N + 64) bytes), grad_mean from gpemu_predict_mean_grad; with variance and grad_variance both NULL
 * emulate_points_grad is emulate_points_mean_grad.  The pair: enqueue starts the variance-gradient batch and returns, collect
 * waits for it and then runs the (much shorter) mean-gradient sweep if grad_mean is asked for.  Errors end in
 * gpemu_host_fatal. */
void emulate_points_grad(emulator_struct *e, gsl_matrix *points, double *mean, double *variance, double *grad_mean, double *grad_variance);
void emulate_points_grad_enqueue(emulator_struct *e, gsl_matrix *points);
void emulate_points_grad_collect(emulator_struct *e, int npoints, double *mean, double *variance, double *grad_mean, double *grad_variance);
/* extension: the joint posterior covariance between the query points (gpemu_predict_cov in gpemu.h): cov[p * npoints + q] is
 * the covariance between the emulator's errors at rows p and q of points (both triangles; its diagonal is emulate_points'
 * variance to rounding), mean (npoints, may be NULL) the posterior mean.  At most 16384 points.  Errors end in
 * gpemu_host_fatal. */
void emulate_points_cov(emulator_struct *e, gsl_matrix *points, double *mean, double *cov);
/* emulate_points_cov in two halves, like emulate_loo_enqueue / _collect: *dev_out is the device buffer the results wait in */
void emulate_points_cov_enqueue(emulator_struct *e, gsl_matrix *points, void **dev_out);
void emulate_points_cov_collect(emulator_struct *e, void *dev, int npoints, double *mean, double *cov);
/* extension: validation on a held-out campaign and joint draws (gpemu_predict_joint_factor / _draw in gpemu.h).  With
 * S = Sigma + diag(noise) (Sigma as emulate_points_cov returns it, noise npoints variances or NULL) factored on the device,
 * S = L L^T, and yobs one observation per row of points (npoints values, or NULL: factor only, for emulate_points_draw):
 *   werr = L^-1 (yobs - mean) (npoints decorrelated errors), *maha = |werr|^2, *logdet = log det S,
 *   *logpdf = -1/2 (maha + logdet + npoints log 2 pi), var = diag S; every output may be NULL.
 * emulate_points_draw returns out[s] = mean + L z[s] for ndraw rows of npoints standard normals, from the factor the last
 * emulate_points_holdout[_enqueue] on e left (kept until e is freed or the next hold-out call on it).  At most 16384 points.
 * Errors, a matrix that is not positive definite among them (coinciding points without noise), end in gpemu_host_fatal. */
void emulate_points_holdout(emulator_struct *e, gsl_matrix *points, const double *yobs, const double *noise, double *mean, double *var,
                            double *werr, double *maha, double *logdet, double *logpdf);
/* in two halves, like emulate_points_cov_enqueue / _collect; nobs = 1 when yobs was given to the enqueue, else 0 */
void emulate_points_holdout_enqueue(emulator_struct *e, gsl_matrix *points, const double *yobs, const double *noise, void **dev_out);
void emulate_points_holdout_collect(emulator_struct *e, void *dev, int npoints, int nobs, double *mean, double *var, double *werr,
                                    double *maha, double *logdet, double *logpdf);
void emulate_points_draw(emulator_struct *e, int ndraw, const double *z, double *out);
/* extension: leave-one-out validation (gpemu_loo in gpemu.h).  mean[i], variance[i] for each of the N training points: what
 * alloc_emulator_struct on the other N - 1 points at the same thetas and emulate_point at x_i return, without refitting */
void emulate_loo(emulator_struct *e, double *mean, double *variance);
/* emulate_loo in two halves, like emulate_points_enqueue / _collect: *dev_out is the device buffer the results wait in */
void emulate_loo_enqueue(emulator_struct *e, void **dev_out);
void emulate_loo_collect(emulator_struct *e, void *dev, double *mean, double *variance);
/* extension: K-fold / leave-group-out validation (gpemu_lgo in gpemu.h).  group[i] in 0 .. ngroups-1 names the group training
 * point i is left out with (-1: never left out).  For every group: what alloc_emulator_struct on the other points at the same
 * thetas predicts JOINTLY at the group's points, without refitting.  mean, variance (required), werr (the group's decorrelated
 * errors; may be NULL): N each in design order, NaN for label -1; maha (squared Mahalanobis distance of the group's errors),
 * logpdf (their joint log predictive density): ngroups each, may be NULL.  A group whose matrix is not positive definite
 * ends in gpemu_host_fatal. */
void emulate_lgo(emulator_struct *e, int ngroups, const int *group, double *mean, double *variance, double *werr, double *maha,
                 double *logpdf);
/* emulate_lgo in two halves, like emulate_loo_enqueue / _collect: *dev_out is the device buffer the results wait in */
void emulate_lgo_enqueue(emulator_struct *e, int ngroups, const int *group, void **dev_out);
void emulate_lgo_collect(emulator_struct *e, void *dev, int ngroups, double *mean, double *variance, double *werr, double *maha,
                         double *logpdf);
/* extension: main effects and Sobol indices of the posterior mean in closed form (gpemu_sens_cov / gpemu_sens_main in gpemu.h;
 * the reference's counterpart is the R code of src/libSA/sa-fns.R, which integrates against a Gaussian input measure -- this
 * integrates over the box [lo_l, hi_l], independent uniform inputs).  Power-exponential covariance only.  lo, hi: nparams each.
 * emulate_sensitivity: *e0 = E[m], *var = V = Var(m), first[j] = V_j = Var(E[m | x_j]), total[j] = VT_j = V - Var(E[m | x_-j])
 * (nparams each; the indices are first[j] / V and total[j] / V).  emulate_main_effects: *e0 and main[j * ngrid + g] =
 * E[m | x_j = grid[j * ngrid + g]], row j of grid holding the values of x_j.  A Matern model, a bad box: gpemu_host_fatal. */
void emulate_sensitivity(emulator_struct *e, const double *lo, const double *hi, double *e0, double *var, double *first, double *total);
void emulate_main_effects(emulator_struct *e, const double *lo, const double *hi, int ngrid, const double *grid, double *e0, double *main);
/* extension: the input measure of the whole family above and below (gpemu_sens_set_measure in gpemu.h).  kind: nparams values,
 * GPEMU_MEASURE_UNIFORM (0, the default) or GPEMU_MEASURE_GAUSS (1), or NULL for all uniform.  From this call on, every
 * emulate_sensitivity*, emulate_main_effects* and emulate_interaction_surface* function reads lo[j] / hi[j] of a Gaussian
 * parameter as its MEAN / STANDARD DEVIATION (sd > 0; hi <= lo is fine there), and a grid value on it may be any finite real.
 * The state lives in the emulator's device context: no struct changes, and it lasts until the emulator_struct is freed or set
 * again.  A kind outside {0, 1}: gpemu_host_fatal.  emulate_sensitivity_measure_multi (below) sets every component. */
void emulate_sensitivity_measure(emulator_struct *e, const int *kind);
/* the covariances behind emulate_sensitivity in two halves, for one emulator (b = a or NULL) or for two on the same design:
 * gpemu_sens_cov_dev is enqueued on a's stream, *dev_out is the device buffer the results wait in; collect returns e0[2] (E0 of
 * a, of b), *cov_all = Cov(m^a, m^b), cov_first[j] = Cov(E[m^a | x_j], E[m^b | x_j]), cov_rest[j] = Cov(E[m^a | x_-j], E[m^b | x_-j]) */
void emulate_sensitivity_enqueue(emulator_struct *a, emulator_struct *b, const double *lo, const double *hi, void **dev_out);
void emulate_sensitivity_collect(emulator_struct *a, void *dev, double *e0, double *cov_all, double *cov_first, double *cov_rest);
/* extension: the emulator's own uncertainty about those quantities (gpemu_sens_post / gpemu_sens_main_var in gpemu.h; the
 * reference's counterpart is the confidence band of src/libSA/trivial-test-2.R).  f is the posterior process, m its mean, and
 * S_u = E Var*[E[f | x_u]].  emulate_sensitivity_post: s = S_none, S_all, S_first[nparams], S_rest[nparams] as the device returns
 * them.  emulate_sensitivity_uncertainty: *var_e0 = S_none = Var*[E0]; *imse = S_all, the box average of the posterior variance
 * (no nugget); the posterior expectations of the variances of f itself, *evar = E*[V] = V + S_all - S_none, efirst[j] = E*[V_j] =
 * V_j + S_j - S_none, etotal[j] = E*[VT_j] = VT_j + S_all - S_{-j}, from one gpemu_sens_cov and one gpemu_sens_post.  A small
 * first[j] with a large efirst[j] - first[j] is an index the design does not resolve.  emulate_main_effects_band: the curves of
 * emulate_main_effects with sd[j * ngrid + g] = sqrt(max(Var*[E[f | x_j = grid[j * ngrid + g]]], 0)); emulate_main_effects_var
 * returns the variances themselves and *var_e0 (may be NULL). */
void emulate_sensitivity_post(emulator_struct *e, const double *lo, const double *hi, double *s /* 2 + 2 nparams */);
void emulate_sensitivity_uncertainty(emulator_struct *e, const double *lo, const double *hi, double *var_e0, double *imse, double *evar,
                                     double *efirst, double *etotal);
void emulate_main_effects_var(emulator_struct *e, const double *lo, const double *hi, int ngrid, const double *grid, double *e0, double *main,
                              double *var, double *var_e0);
void emulate_main_effects_band(emulator_struct *e, const double *lo, const double *hi, int ngrid, const double *grid, double *e0, double *main,
                               double *sd);
/* extension: where to put the next model run (gpemu_design_gain in gpemu.h).  gain[q] = how much *imse of
 * emulate_sensitivity_uncertainty drops when the design gets one more run at points[q] (npoints x nparams, row-major), the
 * hyper-parameters as they are; num and var (either may be NULL) its numerator E_x[c*(x, x*)^2] and the variance the run would be
 * observed with.  lo / hi and the measure as in the emulate_sensitivity* family. */
void emulate_design_gain(emulator_struct *e, const double *lo, const double *hi, int npoints, const double *points, double *gain,
                         double *num, double *var);
/* extension: a batch of nbatch runs chosen greedily among the candidates (gpemu_design_batch in gpemu.h): pick_out[j] the index
 * of pick j, gain_out[j] the further drop of *imse by it, conditional on the picks before it -- the sum of the first j is the
 * drop by all of them.  1 <= nbatch <= min(npoints, 256), npoints <= 16384.  emulate_design_batch_components: the same for n
 * emulators on one design that one run observes together (the components of a multi-output model), the quantity maximised
 * being sum_c weight[c] gain_c (weight NULL: all 1). */
void emulate_design_batch(emulator_struct *e, const double *lo, const double *hi, int npoints, const double *points, int nbatch,
                          int *pick_out, double *gain_out);
void emulate_design_batch_components(emulator_struct **es, int n, const double *weight, const double *lo, const double *hi, int npoints,
                                     const double *points, int nbatch, int *pick_out, double *gain_out);
/* extension: where to put the next model run when what matters is a REGION, given as weighted points (gpemu_design_target_set /
 * _gain in gpemu.h): chain samples of the posterior, the points history matching left standing, quadrature nodes.
 * emulate_design_target_set keeps the ntargets points (ntargets x nparams, row-major; weight NULL: 1 / ntargets each, used as
 * given otherwise) on the emulator and returns *target_var = sum_s w_s v(x_s) and var_t[s] = v(x_s), the latent posterior
 * variance at the targets (either may be NULL); emulate_design_target_gain returns gain[q], how much *target_var drops when the
 * design gets one more run at points[q], the hyper-parameters as they are, with its numerator num = sum_s w_s c*(x_s, x*)^2 and
 * the variance var the run would be observed with (either may be NULL).  Every covariance function; 1 <= ntargets <= 65536.
 * The targets stay resident on the emulator's device, 8 S' (N' + 2 * 64 + nparams + 2) bytes with S' and N' the numbers of targets
 * and training points rounded up to 64 (4 GB at 65536 targets and 8192 points), until emulate_design_target_release, the next
 * emulate_design_target_set or the end of the emulator; a gain call after the release is an error. */
void emulate_design_target_release(emulator_struct *e);
void emulate_design_target_set(emulator_struct *e, int ntargets, const double *targets, const double *weight, double *target_var,
                               double *var_t);
void emulate_design_target_gain(emulator_struct *e, int npoints, const double *points, double *gain, double *num, double *var);
/* extension: second-order Sobol indices and interaction surfaces in closed form (gpemu_sens_pairs / gpemu_sens_pairs_post /
 * gpemu_sens_joint in gpemu.h).  total[j] > first[j] says that parameter j interacts; these say with which parameter.  Pairs j < k
 * are numbered p = j (2 nparams - j - 1) / 2 + (k - j - 1), npairs = nparams (nparams - 1) / 2; nparams >= 2.
 * emulate_sensitivity_pairs: vpair[p] = V_jk = Var(E[m | x_j, x_k]) and inter[p] = V_jk - V_j - V_k, the interaction variance (the
 * second-order index is inter[p] / V).  _enqueue / _collect: the covariances Cov(E[m^a | x_j, x_k], E[m^b | x_j, x_k]) in two halves
 * for one emulator (b = a or NULL) or two on the same design, as emulate_sensitivity_enqueue / _collect.
 * emulate_sensitivity_pairs_post: s_pair[p] = S_u for u = {j, k}.  emulate_sensitivity_pairs_uncertainty: the posterior expectations
 * evpair[p] = E*[V_jk] = V_jk + S_jk - S_none and einter[p] = E*[V_jk - V_j - V_k] = inter[p] + S_jk - S_j - S_k + S_none.
 * emulate_interaction_surface: for one pair j != k and ngrid values of each coordinate, *e0, joint[a * ngrid + b] =
 * E[m | x_j = gj[a], x_k = gk[b]] and inter[a * ngrid + b] = joint - main_j - main_k + E0, the interaction effect (may be NULL),
 * summed without ever forming the large values it is the difference of. */
void emulate_sensitivity_pairs(emulator_struct *e, const double *lo, const double *hi, double *vpair, double *inter);
void emulate_sensitivity_pairs_enqueue(emulator_struct *a, emulator_struct *b, const double *lo, const double *hi, void **dev_out);
void emulate_sensitivity_pairs_collect(emulator_struct *a, void *dev, double *cov_pair);
void emulate_sensitivity_pairs_post(emulator_struct *e, const double *lo, const double *hi, double *s_pair);
void emulate_sensitivity_pairs_uncertainty(emulator_struct *e, const double *lo, const double *hi, double *evpair, double *einter);
void emulate_interaction_surface(emulator_struct *e, const double *lo, const double *hi, int j, int k, int ngrid, const double *gj,
                                 const double *gk, double *e0, double *joint, double *inter);

/* ---- multi_modelstruct.h / multivar_support.h ---------------------------------- */
multi_modelstruct *alloc_multimodelstruct(gsl_matrix *xmodel_in, gsl_matrix *training_matrix_in, int cov_fn_index,
                                          int regression_order, double varfrac);
void gen_pca_decomp(multi_modelstruct *m, double vfrac);
void gen_pca_model_array(multi_modelstruct *m);
void dump_multi_modelstruct(FILE *fptr, multi_modelstruct *m);
multi_modelstruct *load_multi_modelstruct(FILE *fptr);
double vector_elt_sum(gsl_vector *vec, int nstop);
void free_multimodelstruct(multi_modelstruct *m);
multi_emulator *alloc_multi_emulator(multi_modelstruct *model);
void free_multi_emulator(multi_emulator *e);
void estimate_multi(multi_modelstruct *m, FILE *outfp);
void emulate_point_multi(multi_emulator *emu, gsl_vector *the_point, gsl_vector *the_mean, gsl_vector *the_variance);
void emulate_point_multi_pca(multi_emulator *emu, gsl_vector *the_point, gsl_vector *the_mean, gsl_vector *the_variance);
/* extension: batched form of the two calls above; outputs are npoints x nt (or x nr) row-major */
void emulate_points_multi(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *var_out);
/* the means alone: npoints x nr (pca_space) or npoints x nt (training_mean + evecs diag(sqrt(evals)) mean_pca,
 * multivar_support.c:118-137) */
void emulate_points_multi_mean(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out);
/* means (npoints x nr or nt, may be NULL) and their gradients: grad_out is npoints x (nr or nt) x nparams; in observable
 * space grad_Y[t][j] = sum_c evecs[t][c] sqrt(evals[c]) grad_c[j], the back-projection of multivar_support.c:118-137 without
 * the training mean */
void emulate_points_multi_mean_grad(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *grad_out);
/* means, variances (npoints x nr or nt) and their gradients (npoints x (nr or nt) x nparams); any output may be NULL, but
 * not all.  In observable space the mean and its gradient as in emulate_points_multi_mean_grad, the variance and its gradient
 * by the reference's variance rule: grad_var_Y[t][j] = sum_c evecs[t][c]^2 evals[c] grad_var_c[j].  All components are started
 * before the first is collected. */
void emulate_points_multi_grad(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *var_out,
                               double *grad_mean_out, double *grad_var_out);
/* the joint posterior covariance between the query points, one npoints x npoints matrix per output: cov_out is nr x npoints x
 * npoints in PCA space (component c's matrix, the bits of emulate_points_cov on it), nt x npoints x npoints in observable space
 * by the reference's variance rule (multivar_support.c:118-157) applied to every element,
 *   cov_Y[t] = sum_c evecs[t][c]^2 evals[c] Sigma_c,
 * whose diagonal is what emulate_points_multi returns as variance (to rounding: that entry sums in another order).  mean_out
 * (may be NULL) is npoints x nr or nt as emulate_points_multi lays it out.  Every component's device call is started before
 * the first is waited for.  Covariances BETWEEN outputs are not modelled here, as they are not in the reference: its PCA
 * components are independent emulators and its rule keeps only each output's own variance. */
void emulate_points_multi_cov(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *cov_out);
/* extension: validation of a multi-output emulator on a held-out campaign.  Y (npoints x nt, observable space; NULL: factor
 * only) is projected into PCA space exactly as gen_pca_decomp builds pca_zmatrix, (Y - training_mean) evecs / sqrt(evals), and
 * every component c is validated on its own column by emulate_points_holdout (all components are started before the first is
 * collected).  noise_pca (nr x npoints, may be NULL): observation variances per component, in PCA space.  Outputs, any may be
 * NULL: mean_out, var_out, werr_out npoints x nr (the layout of emulate_points_multi in PCA space); maha_out, logdet_out,
 * logpdf_out nr values; *logpdf_sum their sum, the joint log density of the projected observations -- the components are
 * independent emulators.  These diagnostics exist in PCA space ONLY: in observable space the covariance of the nt outputs at a
 * point, sum_c F_tc F_uc Sigma_c, has rank nr and is singular whenever nr < nt, so it has no Cholesky factor, no Mahalanobis
 * distance and no density. */
void emulate_points_multi_holdout(multi_emulator *emu, gsl_matrix *points, const double *Y, const double *noise_pca, double *mean_out,
                                  double *var_out, double *werr_out, double *maha_out, double *logdet_out, double *logpdf_out,
                                  double *logpdf_sum);
/* joint draws at the npoints points of the last emulate_points_multi_holdout: z is nr x ndraw x npoints standard normals (component
 * c draws with z[c] from its own factor), out is ndraw x npoints x nr in PCA space or ndraw x npoints x nt in observable space:
 * training_mean + evecs diag(sqrt(evals)) draw_pca through gpemu_host_backproject (not squared, mean added) */
void emulate_points_multi_draw(multi_emulator *emu, int pca_space, int npoints, int ndraw, const double *z, double *out);
/* extension: implausibility and calibration likelihood against observations (gpemu_calib_* in gpemu.h; the
 * reference does this in R only: libRbind/implausOverDesign.R).  An observation set: z (nt values) with either standard
 * deviations sd (nt) or a covariance cov (nt x nt, row-major, replaces sd^2) -- exactly one of the two --, and optionally a
 * relative model error rel (nt, >= 0: the reference's errModel.sys; NULL: none).  alloc_observations builds A = pca_evecs_r
 * sqrt(pca_evals_r) and ybar = training_mean exactly as gpemu_host_backproject does (the factor u * sqrt(lam) formed first),
 * runs the projection and keeps its tables on the device of component 0.  nr <= 16, nt <= 1024; beyond, a malformed set or a
 * covariance that is not positive definite: a message and the layer's exit.  gpemu_host_observations_misfit: c_perp, the
 * misfit no parameter value can remove, and its degrees of freedom nt - nr. */
typedef struct gpemu_observations gpemu_observations;
gpemu_observations *alloc_observations(multi_modelstruct *m, const double *z, const double *sd, const double *cov, const double *rel);
void free_observations(gpemu_observations *obs);
void gpemu_host_observations_misfit(const gpemu_observations *obs, double *c_perp, int *dof);
/* the reference's confidence rule (implausOverDesign.R): a relative error sig / qnorm(1 - sig / 2) for 0 < sig < 1, NaN otherwise */
double gpemu_host_confidence_to_rel(double sig);
/* stat_out: npoints x 5 per point {chi2, joint log density, largest, second and third largest per-output implausibility};
 * worst_out (npoints, may be NULL): the output of the largest.  The points go up once per device, every component's
 * gpemu_predict_batch_dev writes its row of a component-major device buffer (all started before the first is waited for; a
 * component on another device has its row moved across through the host), then one evaluation launch; 5 npoints doubles and
 * npoints ints come back.  No npoints x nt array exists anywhere.  Any npoints (blocks of 262144). */
void emulate_points_multi_implausibility(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double *stat_out, int *worst_out);
/* the same with the selection on the device: point q is kept iff chi2 <= cut_chi2 and the level-th largest implausibility
 * (level 1, 2 or 3) <= cut_I; INFINITY disables a cut, a NaN is never kept.  idx_out (room for npoints) receives the kept
 * indices in ascending order, stat_out (room for npoints x 5) their statistics, *nkeep their number: only these are downloaded. */
void emulate_points_multi_nonimplausible(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double cut_chi2, int level,
                                         double cut_I, int *idx_out, double *stat_out, int *nkeep);
/* ... and the kept points' worst outputs (worst_out: room for npoints, may be NULL) */
void emulate_points_multi_nonimplausible_worst(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double cut_chi2, int level,
                                               double cut_I, int *idx_out, double *stat_out, int *worst_out, int *nkeep);
/* the gradient of the joint log density with respect to the points' coordinates (gpemu_calib_grad in gpemu.h):
 * grad_logpdf_out[p * nparams + j] = d logpdf(x_p) / d x_j, grad_chi2_out (may be NULL) likewise for chi2, in the units of
 * `points` -- the units emulate_points_multi_grad returns --; stat_out (npoints x 5, may be NULL) as
 * emulate_points_multi_implausibility returns it, bit for bit (its sweep then runs as well).  The points go up once per
 * device; every component's mean-gradient and variance-gradient sweeps write component-major device buffers on the observation
 * set's device (all started before the first is waited for; a component on another device crosses through the host); then one
 * gradient launch; npoints x nparams doubles per array come back.  Any npoints, in blocks of 16384: the gradient buffers,
 * 2 nr npoints nparams doubles, bound the block -- 152 MB on the observation set's device at nr = 16, nparams = 32.  The
 * per-output implausibilities are not differentiated (a max-type statistic).  A NULL argument or an observation set of another
 * model: a message with this entry's name and the layer's exit. */
void emulate_points_multi_logpdf_grad(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double *stat_out,
                                      double *grad_logpdf_out, double *grad_chi2_out);
void gpemu_host_calib_grad_block(const void *key, emulator_struct **es, int nr, int np, int d, const double *q, double *stat,
                                 double *glogpdf, double *gchi2);
/* (device_bridge.c: the observation set's device context and one block of points) */
void gpemu_host_calib_setup(const void *key, int nt, int nr, const double *ybar, const double *A, const double *z, const double *S,
                            const double *sd, const double *rel);
void gpemu_host_calib_block(const void *key, emulator_struct **es, int nr, int np, int d, const double *q, int select, double cut_chi2,
                            int level, double cut_I, double *stat, int *worst, int *idx, int *nkeep);
/* extension: posterior samples of the parameters by the affine-invariant ensemble sampler on the device (gpemu_calib_sample in
 * gpemu.h; sample.c).  Log posterior = the joint log density of obs at the point + the log of an independent
 * prior per parameter: lo, hi, kind (nparams each) in the convention of emulate_sensitivity_measure -- kind NULL: all uniform on
 * [lo, hi]; for GPEMU_MEASURE_GAUSS (1) lo is the mean and hi the standard deviation.  args: the run (nwalkers even, nwalkers / 2
 * >= nparams + 1; nsteps; burn and thin count global steps; seed; first_step; the stretch scale a > 1).  x0: nwalkers x nparams
 * starts, or NULL: drawn from the prior with the sampler's generator at counters (k, j, 0, 2) for parameter j of walker k --
 * uniform: lo + u1 (hi - lo); Gaussian: mean + sd sqrt(-2 ln u1) cos(2 pi u2) -- (gpemu_host_sample_starts, no device).
 * Outputs, in the units of the points: trace_x (nrec x nwalkers x nparams) and trace_lp (nrec x nwalkers), nrec =
 * gpemu_host_sample_nrec(args) records; x_end (nwalkers x nparams, may be NULL), what a following call with first_step =
 * first_step + nsteps starts from; *accept_out the accepted fraction of the call's proposals; summary_out (may be NULL) 6 rows
 * of nparams over the recorded samples: mean, standard deviation (divisor n), the 2.5 / 50 / 97.5 % quantiles (linear
 * interpolation between order statistics, numpy's default), and the integrated autocorrelation time tau of the ensemble-mean
 * series in recorded steps.  gpemu_host_autocorr_time: tau(M) = 1 + 2 sum_{t=1..M} rho(t) with Sokal's window, the smallest
 * M >= 5 tau(M) (the last M when none is); returns 0, or 1 (tau = NaN) for a NULL pointer or n < 1; a constant series has tau 1.
 * A start with a non-finite log posterior, a bad prior or run, an observation set of another model: a message and the layer's
 * exit; so do components on different devices (not built). */
/* (the fields of gpemu_sample_args in gpemu.h, which this header does not need) */
typedef struct gpemu_host_sample_args {
	int nwalkers, nsteps, burn, thin;
	unsigned long long seed, first_step;
	double a;
} gpemu_host_sample_args;
int gpemu_host_sample_nrec(const gpemu_host_sample_args *args);
void gpemu_host_sample_starts(unsigned long long seed, int nwalkers, int nparams, const int *kind, const double *lo, const double *hi,
                              double *x0_out);
int gpemu_host_autocorr_time(const double *series, int n, double *tau);
void emulate_sample_posterior_multi(multi_emulator *emu, gpemu_observations *obs, const double *lo, const double *hi, const int *kind,
                                    const gpemu_host_sample_args *args, const double *x0, double *trace_x, double *trace_lp,
                                    double *x_end, double *accept_out, double *summary_out);
/* (device_bridge.c: the prior onto the observation set's context, then the run) */
void gpemu_host_calib_sample(const void *key, emulator_struct **es, int nr, int d, const int *kind, const double *lo, const double *hi,
                             const gpemu_host_sample_args *args, const double *x0, double *trace_x, double *trace_lp, double *x_end,
                             double *lp_end, int *naccept, int *nrec);
/* extension: leave-one-out at every training point of a multi-output emulator; outputs are nmodel_points x nr in PCA space,
 * or nmodel_points x nt in observable space (every component's leave-one-out result through the same back-projection) */
void emulate_loo_multi(multi_emulator *emu, int pca_space, double *mean_out, double *var_out);
/* extension: K-fold / leave-group-out validation of a multi-output emulator, the same groups for every component (all components
 * are started before the first is waited for).  mean_out, var_out as emulate_loo_multi lays them out (NaN rows for label -1);
 * maha_out, logpdf_out (may be NULL): nr x ngroups, component-major, in PCA space only, as for the hold-out mode */
void emulate_lgo_multi(multi_emulator *emu, int pca_space, int ngroups, const int *group, double *mean_out, double *var_out,
                       double *maha_out, double *logpdf_out);
/* extension: sensitivity analysis of a multi-output emulator over the box [lo, hi].  Outputs per output (nr in PCA space, nt in
 * observable space): e0_out, var_out one value each; first_out, total_out nparams values each, output-major.  In PCA space the
 * components are analysed one by one.  In observable space y_t = training_mean[t] + sum_c B_tc m_c with B_tc = evecs[t][c]
 * sqrt(evals[c]), and the components are NOT independent under the input measure (they are functions of the same x), so
 *   Var_u(y_t) = sum_{c,c'} B_tc B_tc' cov_u(c, c'):
 * all nr (nr + 1) / 2 pairs of components are analysed (two device contexts each), every pair started before the first is
 * collected, and contracted on the host.  The squared rule of gpemu_host_backproject (sum_c B_tc^2 var_c) is for the emulator's
 * posterior uncertainty, where the components ARE independent; here it would drop every cross term. */
void emulate_sensitivity_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *e0_out, double *var_out,
                               double *first_out, double *total_out);
/* the input measure of every *_multi sensitivity function of emu from now on: emulate_sensitivity_measure on every component
 * (the kinds are per parameter, the same for all components); lo / hi then mean mean / sd on a Gaussian parameter */
void emulate_sensitivity_measure_multi(multi_emulator *emu, const int *kind);
/* main-effect curves of every output: main_out is (nparams x ngrid) x (nr or nt), element ((j * ngrid + g) * nout + t); e0_out
 * nr or nt values.  Observable space by the mean half of the rule (linear in the components), training mean added. */
void emulate_main_effects_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int ngrid, const double *grid,
                                double *e0_out, double *main_out);
/* the emulator-uncertainty terms per output: var_e0_out, imse_out, evar_out one value each, efirst_out, etotal_out nparams values
 * each, output-major, as emulate_sensitivity_uncertainty defines them.  In observable space the two halves take OPPOSITE rules --
 * the opposite of the trap described at emulate_sensitivity_multi.  The plug-in part (V, V_j, VT_j of the posterior mean) keeps its
 * cross terms between components, which are functions of the same random input.  The S terms are posterior variances, and the PCA
 * components are independent a posteriori, so they take the squared rule of gpemu_host_backproject: S_u(y_t) = sum_c B_tc^2 S_u^c,
 * with no cross terms.  emulate_main_effects_band_multi: main_out as emulate_main_effects_multi, sd_out in the same layout, the
 * square root of the squared rule applied to the components' variances. */
void emulate_sensitivity_uncertainty_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *var_e0_out,
                                           double *imse_out, double *evar_out, double *efirst_out, double *etotal_out);
void emulate_main_effects_band_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int ngrid, const double *grid,
                                     double *e0_out, double *main_out, double *sd_out);
/* the expected drop of every output's IMSE by one more run at each of npoints candidates (points: npoints x nparams, row-major):
 * gain_out[q * nout + t], nout = nt (nr in PCA space).  One run observes every component and the components are independent a
 * posteriori, so the result takes the squared rule of gpemu_host_backproject, gain(y_t) = sum_c B_tc^2 gain_c; total_out[q]
 * (may be NULL) is its sum over the outputs. */
void emulate_design_gain_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int npoints, const double *points,
                               double *gain_out, double *total_out);
/* a batch of nbatch runs chosen greedily (emulate_design_batch_components over the PCA components): every pick maximises what
 * total_out of emulate_design_gain_multi would be given the picks before it, sum_c weight_c gain_c with weight_c = sum_t B_tc^2
 * from gpemu_host_backproject's squared rule (all 1 in PCA space).  pick_out[j]: the candidate's index, gain_out[j]: the drop
 * of the summed IMSE by pick j. */
void emulate_design_batch_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int npoints, const double *points,
                                int nbatch, int *pick_out, double *gain_out);
/* the same for a region given as ntargets weighted points (emulate_design_target_set / _gain): the targets go to every PCA
 * component, and both results take the squared rule, gain(y_t) = sum_c B_tc^2 gain_c and target_var(y_t) = sum_c B_tc^2
 * target_var_c.  gain_out[q * nout + t]; total_out[q] (may be NULL) its sum over the outputs; target_var_out[t] (may be NULL).
 * Every component's targets are released again before the next component takes its own: nothing of the call stays resident. */
void emulate_design_target_gain_multi(multi_emulator *emu, int pca_space, int ntargets, const double *targets, const double *weight,
                                      int npoints, const double *points, double *gain_out, double *total_out, double *target_var_out);
/* second order per output: vpair_out, inter_out, evpair_out, einter_out are npairs values each, output-major, as
 * emulate_sensitivity_pairs / _uncertainty define them.  Observable space exactly as for emulate_sensitivity_multi /
 * _uncertainty_multi: the plug-in half keeps all cross terms between components, sum_{c,c'} B_tc B_tc' cov_pair(c, c') (every pair
 * of components started before the first is collected); the S half takes the squared rule.  The surface is linear in the
 * components: joint_out and inter_out (may be NULL) are (ngrid x ngrid) x (nr or nt), element ((a * ngrid + b) * nout + t), the
 * training mean added to joint_out and e0_out and not to inter_out. */
void emulate_sensitivity_pairs_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *vpair_out,
                                     double *inter_out);
void emulate_sensitivity_pairs_uncertainty_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *evpair_out,
                                                 double *einter_out);
void emulate_interaction_surface_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int j, int k, int ngrid,
                                       const double *gj, const double *gk, double *e0_out, double *joint_out, double *inter_out);

/* ---- libRbind/rbind.h: the batched likelihood entry point, R-free (rbind.c:626-724) ---------------- */
void callEvalLhoodList(double *xmodel_in, int *nparams_in, double *pointList_in, int *nevalPoints_in,
                       double *training_in, int *nmodelPoints_in, int *nthetas_in, double *answer,
                       int *cov_fn_index_in, int *regression_order_in);
void callEstimate(double *xmodel_in, int *nparams_in, double *training_in, int *nmodelpts, int *nthetas_in, double *final_thetas,
                  int *use_fixed_nugget, double *fixed_nugget_in, int *cov_fn_index_in, int *regression_order_in);
void callEmulateAtList(double *xmodel_in, int *nparams_in, double *points_in, int *nemupoints, double *training_in,
                       int *nmodelpts, double *thetas_in, int *nthetas_in, double *final_emulated_y,
                       double *final_emulated_variance, int *cov_fn_index_in, int *regression_order_in);
void callEmulateAtPt(double *xmodel_in, int *nparams_in, double *point_in, double *training_in, int *nmodelpts,
                     double *thetas_in, int *nthetas_in, double *final_emulated_y, double *final_emulated_variance,
                     int *cov_fn_index_in, int *regression_order_in);
/* one emulator (or nydims of them on one design) kept between calls -- rbind.c:299-600 */
void setupEmulateMC(double *xmodel_in, int *nparams_in, double *training_in, int *nmodelpts, double *thetas_in, int *nthetas_in,
                    int *cov_fn_index_in, int *regression_order_in);
void callEmulateMC(double *point_in, double *mean_out, double *var_out);
void freeEmulateMC(void);
void setupEmulateMCMulti(double *xmodel_in, int *nparams_in, double *training_in, int *nydims_in, int *nmodelpts_in,
                         double *thetas_in, int *nthetas_in, int *cov_fn_index_in, int *regression_order_in);
void callEmulateMCMulti(double *point_in, int *nydims_in, double *final_mean, double *final_var);
void freeEmulateMCMulti(int *nydims_in);

/* ---- knobs of this implementation (not in the reference) ------------------------ */
/* How the layer ends the process where the reference calls exit(1) (fatal.c): single entry -- the first caller wins, later
 * ones sleep --, message, flush, _exit(status): no atexit handler or static destructor (the HIP runtime's) runs beside the
 * host threads that are still inside device calls.  gpemu_host_fatal prints its message INSIDE the gate (one message however
 * many threads fail together) and leaves with EXIT_FAILURE. */
void gpemu_host_exit(int status) __attribute__((noreturn));
void gpemu_host_fatal(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));
void gpemu_host_on_exit(void (*hook)(int status));
void gpemu_host_set_device(int device);          /* pin the whole process to ONE HIP device (before the first device call) */
/* device slots: GPEMU_DEVICES=0,1,... (repeats allowed), else every visible device, else the pinned one.  Independent
 * work (PCA components, restart groups, component emulators) is dealt to the slots; a thread working for a slot
 * declares it with gpemu_host_thread_device(device) and every context created from that thread lives there. */
int gpemu_host_device_slots(void);
int gpemu_host_slot_device(int slot);
void gpemu_host_thread_device(int device);       /* -1: back to slot 0 */
int gpemu_host_thread_device_get(void);
int gpemu_host_device(void);                     /* device a context created by the calling thread would get */
/* n searches run side by side on the calling thread's device (the component threads of estimate_multi): the search this
 * thread starts sizes its lock-step groups for 1/n of the device's free memory */
void gpemu_host_thread_share(int n);
int gpemu_host_thread_share_get(void);
/* device bytes ONE lock-step group of `lockstep` value+gradient evaluations at nmodel_points holds (optimizer.c) */
double gpemu_host_group_bytes(int nmodel_points, int lockstep);
void gpemu_host_set_seed(unsigned long seed);    /* 0 = /dev/urandom as the reference (estimate_threaded.c:159) */
void gpemu_host_set_search(int nthreads, int restarts_per_job);   /* defaults: 1 thread (1 GPU stream), 50 restarts */
/* what the BFGS runs did so far in this process: runs, runs that ended at |g| < 0.1, runs that ended with "no progress",
 * line searches that fell back to "lowest trial value" (no Wolfe point), |g| at the end of the winning run of the last search */
void gpemu_host_search_stats(long *runs, long *converged, long *noprogress, long *ls_fallbacks, double *best_gnorm);
/* device evaluations of this process so far: value-only, value+gradient, requests answered from a caller's cache of its
 * last results, lock-step rounds and the requests they carried (GPEMU_SEARCH_STATS=1 prints the figures of a search) */
void gpemu_host_eval_stats(long *value_evals, long *valgrad_evals, long *cached, long *rounds, long *round_elements);
/* the corrected forms of gpemu.h (GPEMU_MODE_EXACT_GRAD = 1, GPEMU_MODE_MATERN_LOG = 2) for the WHOLE host layer: first
 * read from GPEMU_EXACT_GRAD / GPEMU_MATERN_FIXED, set here (the CLI's --exact_gradient / --matern_fixed; a snapshot that
 * records the log-scale mode), applied to every device context the layer holds or creates */
int gpemu_host_modes(void);
void gpemu_host_set_modes(int flags);
void gpemu_host_release(void *params_or_emulator); /* drop the device context cached for a params / emulator pointer */
/* the PCA -> observable rule of the emulate_*_multi entries (multivar_support.c:118-157), host arithmetic only (multi.c):
 *   out[q][t][j] = (add_mean && j == 0 ? training_mean[t] : 0) + sum_c F[t][c] * in[q][c][j],   q < nrows, j < width
 * F = evecs * sqrt(evals) (squared = 0: means, mean gradients) or evecs^2 * evals (squared = 1: variances, their gradients,
 * covariances; a component-major [c][M x M] buffer is nrows = 1, width = M x M).  in is nrows x nr x width, out nrows x nt x
 * width, both row-major and distinct.  The sum runs over c in index order from 0.0; the training mean is added last. */
void gpemu_host_backproject(const multi_modelstruct *m, int squared, int add_mean, size_t nrows, size_t width,
                            const double *in, double *out);
/* the observable -> PCA projection of emulate_points_multi_holdout, host arithmetic only (multi.c): Y is np x nt, z comes back
 * component-major, z[c * np + p] = (sum_t (Y[p][t] - training_mean[t]) evecs[t][c]) * (1 / sqrt(evals[c])), the sum over t in
 * index order from 0.0 -- the arithmetic gen_pca_decomp builds pca_zmatrix with */
void gpemu_host_project_observations(const multi_modelstruct *m, size_t np, const double *Y, double *z);
/* lock-step group: n restart threads (one struct estimate_thetas_params each, same model) share one device context;
 * their concurrent evalFnMulti / gradFnMulti / evalFnGradMulti / estimateSigmaFull calls are gathered into device
 * batches.  A member's thread calls gpemu_host_group_leave(params) when it will make no further calls. */
/* how estimate_thetas_threaded deals a run list to threads, groups and slots (pure arithmetic; optimizer.c) */
int gpemu_host_plan_groups(int total_runs, int lockstep, int per_slot, int nslots, int *nthreads_out, int *lo, int *hi, int *slot,
                           int cap);
void *gpemu_host_group_create(struct estimate_thetas_params **members, int n);
void gpemu_host_group_leave(void *params);
void gpemu_host_group_destroy(void *group);

/* one process per GPU (ranks.c): GPEMU_RANK / GPEMU_WORLD_SIZE / GPEMU_LOCAL_RANK / GPEMU_RENDEZVOUS_DIR.  estimate_multi deals
 * the PCA components, estimate_thetas_threaded (single-output models) the runs of the run list to the ranks; the one
 * collective is an all-gather of a few doubles per rank (RCCL: gpemu_rccl_allgather; GPEMU_GATHER=file for ranks that share
 * a device).  Rank 0 writes the snapshot; every rank ends with the full model. */
/* 1 when alloc_emulator_struct would refuse the model at its present thetas ("trying to cholesky a non postive def matrix"),
 * without exiting: estimate_thetas warns with it when a search has ended on a numerically singular model */
int gpemu_host_emulator_setup_fails(modelstruct *model);
int gpemu_host_world_size(void);
int gpemu_host_rank(void);
void gpemu_host_rank_device(void);
void gpemu_host_allgather(const double *send, int count, double *recv);
/* this rank's part in the run is over (after the last gather; idempotent, also run by a regular exit()): the RCCL communicator
 * goes, the exit is marked as a regular one, rank 0 removes the run's files from the rendezvous directory */
void gpemu_host_ranks_finish(void);

/* interactive_mode's request/response loop (src/interactive_emulator.c:398-440) as a reader -> device -> writer pipeline
 * (interactive_io.c): reads points of nparams numbers from fd_in -- text, the reference's fscanf("%lf%*c") framing, or raw
 * doubles (binary != 0: the reference's BINARY_INTERACTIVE_MODE framing, :418-432) --, hands the points that are already
 * waiting to `fn` as one batch (mean / var: npoints x nout, row-major) and writes nprint (mean, variance) pairs per point
 * ("%.17f\n" each, or raw doubles; pairs beyond nout are zeros) in input order, one flush per batch.  A lone point is
 * answered at once.  Returns 0 at end of input, -2 when fd_out failed. */
typedef void (*gpemu_points_fn)(void *user, int npoints, const double *points, double *mean, double *var);
struct gpemu_io_stats { long points, batches; int max_batch; double parse_seconds, compute_seconds, format_seconds, wall_seconds; };
int gpemu_host_interactive_loop(int fd_in, int fd_out, int nparams, int nout, int nprint, int binary, gpemu_points_fn fn,
                                void *user, struct gpemu_io_stats *stats);
/* the same with nextra further values per point behind its nprint pairs ("%.17f\n" each, or raw doubles): fn_extra is called
 * right after fn on the same batch and fills extra (npoints x nextra, row-major).  nextra = 0 with fn_extra = NULL is
 * gpemu_host_interactive_loop, byte for byte.  -1 for nextra < 0 or a function without values / values without a function. */
typedef void (*gpemu_points_extra_fn)(void *user, int npoints, const double *points, double *extra);
int gpemu_host_interactive_loop_extra(int fd_in, int fd_out, int nparams, int nout, int nprint, int binary, gpemu_points_fn fn,
                                      int nextra, gpemu_points_extra_fn fn_extra, void *user, struct gpemu_io_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
