/*
 * gpemu.h -- C-ABI of the MI355X (gfx950) device library for the
 * MADAIEmulator GP hot path (libgpemu_hip.so).
 *
 * Plain C: opaque handle, plain pointers and sizes, int status returns.  No
 * GSL and no torch types cross this boundary.  Every entry point names the
 * reference interface it stands in for (paths relative to the reference's
 * src/ directory).  All matrices are row-major, element (i,j) at a[i*ld+j]
 * (the gsl_matrix layout); all arithmetic is IEEE fp64.
 *
 * Threading: a gpemu_ctx owns one HIP stream and its own HBM workspace; one
 * ctx per host thread (this is what the reference's per-thread
 * estimate_thetas_params deep copy becomes, libEmu/estimate_threaded.c:57-68).
 * Different ctx objects may be used concurrently.
 *
 * There is no CPU fallback: every compute entry fails with
 * GPEMU_ERR_NO_DEVICE / GPEMU_ERR_HIP when no gfx950 device is usable.
 */
#ifndef GPEMU_H
#define GPEMU_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* covariance-function index, optstruct.h:12-14 */
#define GPEMU_POWEREXP 1
#define GPEMU_MATERN32 2
#define GPEMU_MATERN52 3

#define GPEMU_MAX_PARAMS 64   /* largest design dimension d accepted */

/* status codes */
#define GPEMU_OK              0
#define GPEMU_ERR_ARG         1   /* bad argument / model not set */
#define GPEMU_ERR_NO_DEVICE   2   /* no HIP device */
#define GPEMU_ERR_HIP         3   /* a HIP runtime call failed; see gpemu_last_error */
#define GPEMU_ERR_NOT_PD      4   /* Cholesky met a pivot <= 0 (GSL_EDOM in the reference) */
#define GPEMU_ERR_REGRESSION  5   /* H^T C^-1 H not positive definite (regression.c:134-160) */
#define GPEMU_ERR_STATE       6   /* call order (e.g. predict before predict_setup) */

typedef struct gpemu_ctx gpemu_ctx;

/* ---- context ------------------------------------------------------- */
int  gpemu_ctx_create(gpemu_ctx **out, int device);
void gpemu_ctx_destroy(gpemu_ctx *ctx);
const char *gpemu_last_error(const gpemu_ctx *ctx);
int  gpemu_ctx_device(const gpemu_ctx *ctx);   /* the HIP device the context was created on, -1 for NULL */
const char *gpemu_version(void);
int  gpemu_device_count(void);
/* free / total HBM of a device in bytes (hipMemGetInfo): the host layer sizes its lock-step groups with it.  A likelihood
 * batch of nb evaluations holds nb * (N + 64) * N * 8 bytes, a value+gradient batch nb * (2 N + 64) * N * 8 plus up to
 * 10 GB of C^-1 corners, per context. */
int  gpemu_device_memory(int device, size_t *free_bytes, size_t *total_bytes);

/* ---- the single collective of a multi-process run (north_star: "one GPU per shard with a single RCCL gather
 * over xGMI at the end"): all-gather of `count` doubles per rank over RCCL -- what the mutex-guarded arg-max of
 * libEmu/estimate_threaded.c:308-313 and the serial component loop of multivar_support.c:20-28 become when the
 * independent restarts / PCA components run one process per GPU (csrc/host/ranks.c).  Host buffers:
 * recv[r * count + i] = rank r's send[i].  librccl is opened at run time; the ncclUniqueId goes from rank 0 to the
 * others through the file `id_path` (a fresh name per call, in a directory every rank can reach).  errbuf (optional)
 * receives the message of a failure. */
int gpemu_rccl_allgather(int device, int rank, int world, const char *id_path, const double *send, int count,
                         double *recv, char *errbuf, size_t errlen);
/* The same gather in three steps, for ranks that meet when they START (csrc/host/ranks.c: the communicator exists before
 * the training begins, so a rank never sits in a rendezvous for as long as the slowest rank trains):
 *   gpemu_rccl_unique_id       rank 0 makes the id (GPEMU_RCCL_ID_BYTES bytes = ncclUniqueId); the caller carries it over
 *   gpemu_rccl_comm_create     every rank joins (ncclCommInitRank, collective); *comm_out is an opaque handle
 *   gpemu_rccl_comm_allgather  ncclAllGather of count doubles per rank on the communicator's own stream, host buffers
 *   gpemu_rccl_comm_destroy    the end of the communicator */
#define GPEMU_RCCL_ID_BYTES 128
int gpemu_rccl_unique_id(void *id_out, char *errbuf, size_t errlen);
int gpemu_rccl_comm_create(int device, int rank, int world, const void *id, void **comm_out, char *errbuf, size_t errlen);
int gpemu_rccl_comm_allgather(void *comm, const double *send, int count, double *recv, char *errbuf, size_t errlen);
void gpemu_rccl_comm_destroy(void *comm);

/* ---- model data (modelstruct.h:28-98: xmodel, training_vector) ------
 * Uploads the N x d design and the N training values to HBM and builds the
 * regression basis H (regression.c:9-67,100-112: nreg = 1 + order*d) there.
 * cov_fn_index is GPEMU_POWEREXP / MATERN32 / MATERN52. */
int gpemu_set_model(gpemu_ctx *ctx, int cov_fn_index, int regression_order,
                    int nmodel_points, int nparams,
                    const double *xmodel /* N*d host */, const double *training_vector /* N host */);
/* replace only the training vector (multi_modelstruct: same design, nr PCA columns) */
int gpemu_set_training(gpemu_ctx *ctx, const double *training_vector);

/* ---- a4: makeCovMatrix_fnptr (libEmu/emulator.c:636-653) -----------
 * Full N x N covariance matrix (both triangles) for the model's design at
 * the full theta vector, written to host memory c_out[N*N]. */
int gpemu_cov_matrix(gpemu_ctx *ctx, const double *thetas, int nthetas, double *c_out);

/* ---- a16: makeKVector_fnptr (libEmu/emulator.c:578-593) ------------
 * k[q*N + i] = cov(x_i, xq_q), entries < 1e-10 clamped to 0; M query rows. */
int gpemu_kvectors(gpemu_ctx *ctx, const double *thetas, int nthetas,
                   int npoints, const double *xq /* M*d host */, double *k_out /* M*N host */);

/* ---- a11: evalFnMulti / a9 estimateSigma / a10 getLogLikelyhood -----
 * (libEmu/maxmultimin.c:288-394, 215-273; libEmu/estimator-fns.c:38-103)
 * One likelihood evaluation at FULL thetas (the reference's evalFnMulti
 * passes theta[0] = 0; the drop-in wrapper does that).  Outputs (any may be
 * NULL):  neg_loglik = -logL with log det = 2*sum(log L_ii);  sigma2 =
 * y.Cinv.(y - H beta)/N;  beta[nreg];  logdet;  quad = r.Cinv.r.
 * *info = 0, or 1-based index of the first pivot <= 0 (then
 * GPEMU_ERR_NOT_PD is returned and the outputs are NaN). */
int gpemu_loglik(gpemu_ctx *ctx, const double *thetas, int nthetas,
                 double *neg_loglik, double *sigma2, double *beta,
                 double *logdet, double *quad, int *info);
/* as above, but only enqueues the device work (no host sync, no outputs):
 * used by the throughput bench to time back-to-back evaluations; follow the
 * last call with gpemu_loglik_collect. */
int gpemu_loglik_enqueue(gpemu_ctx *ctx, const double *thetas, int nthetas);
int gpemu_loglik_collect(gpemu_ctx *ctx, double *neg_loglik, double *sigma2, double *beta,
                         double *logdet, double *quad, int *info);

/* ---- a11 over a list of thetas: callEvalLhoodList (libRbind/rbind.c:626-724) and the
 * independent restarts of estimate_thetas_threaded (libEmu/estimate_threaded.c:101-113).
 * nb likelihood evaluations of the SAME model at nb theta vectors (thetas = nb rows of
 * nthetas), factored in lock-step on the device: every kernel handles all nb matrices, so
 * the latency-bound panel chain is paid once per batch.  Outputs are arrays of nb (beta:
 * nb*nreg), any may be NULL; status[b] is what gpemu_loglik would have returned for element b
 * (GPEMU_OK / GPEMU_ERR_NOT_PD / GPEMU_ERR_REGRESSION) and the function itself returns
 * GPEMU_OK when the batch ran.  Workspace: nb * (N+64) * N * 8 bytes of HBM. */
#define GPEMU_MAX_BATCH 64
int gpemu_loglik_batch(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas,
                       double *neg_loglik, double *sigma2, double *beta, double *logdet,
                       double *quad, int *info, int *status);
int gpemu_loglik_batch_enqueue(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas);
int gpemu_loglik_batch_collect(gpemu_ctx *ctx, int nb, double *neg_loglik, double *sigma2,
                               double *beta, double *logdet, double *quad, int *info, int *status);
/* the results of the last GPEMU_RESULT_RING enqueued batches stay readable (pinned ring): `back` = 0 is the newest
 * batch, 1 the one before, ...  Waits for that batch only, so a throughput caller collects EVERY batch while the
 * following ones are already running (what a restart pool consuming its results does). */
#define GPEMU_RESULT_RING 4
int gpemu_loglik_batch_collect_back(gpemu_ctx *ctx, int back, int nb, double *neg_loglik, double *sigma2,
                                    double *beta, double *logdet, double *quad, int *info, int *status);

/* ---- modes (SURVEY App. C2-C4 policy: literal by default, corrected forms behind flags) ----------------------
 * GPEMU_MODE_EXACT_GRAD: gpemu_grad / gpemu_loglik_grad[_batch] return the TRUE gradient of the value gpemu_loglik
 *   returns at theta[0] = 0, d(-logL)/dtheta_k = 1/2 tr(C^-1 dC_k) - 1/2 r^T C^-1 dC_k C^-1 r with r = y - H beta and
 *   the true dC/dtheta (pow-exp: full kernel value times D_k^2 e^{-2 theta_k}; Matern: analytic in log rho; nugget
 *   wherever the nugget rule adds it) instead of the reference's literal formulas (emulator.c:173-209 keeps one
 *   coordinate's factor; maxmultimin.c:514,532,594 scale by sigma^2 and use y).
 * GPEMU_MODE_MATERN_LOG: the Matern kernels take amplitude and nugget on the log scale (amp = e^theta0, nug =
 *   e^theta1) like the pow-exp kernel, instead of raw (emulator.c:355-356,448-449) -- with the raw form evalFnMulti's
 *   theta[0] = 0 (maxmultimin.c:311) makes C = theta1 * I and the reference cannot train a Matern model at all.
 *   Applies to fill, likelihood and prediction alike; a snapshot trained with it must be queried with it.
 * Matern gradients exist only with both flags.  Defaults come from the environment when the context is created
 * (GPEMU_EXACT_GRAD=1, GPEMU_MATERN_FIXED=1); both off = the reference's literal behaviour. */
#define GPEMU_MODE_EXACT_GRAD 1
#define GPEMU_MODE_MATERN_LOG 2
int gpemu_set_mode(gpemu_ctx *ctx, int flags);
int gpemu_get_mode(const gpemu_ctx *ctx);

/* ---- a12: gradFnMulti + getGradientCn (maxmultimin.c:416-550,571-608)
 * grad[nthetas-1] as the reference defines it (literal formulas, SURVEY
 * App. A.3): thetas are the FULL vector with theta[0] ignored (set to 0 for
 * the matrix, replaced by log sigma^2 for the amplitude factor). */
int gpemu_grad(gpemu_ctx *ctx, const double *thetas, int nthetas, double *grad, int *info);
/* a13: evalFnGradMulti (maxmultimin.c:615-618): value and gradient from ONE factorisation (the reference
 * fills and factors twice).  neg_loglik is the evalFnMulti value (theta[0] taken as 0). */
int gpemu_loglik_grad(gpemu_ctx *ctx, const double *thetas, int nthetas, double *neg_loglik, double *sigma2,
                      double *beta, double *grad, int *info);
/* a13 over a list of thetas: the value+gradient pairs the independent restarts of maxWithMultiMin
 * (libEmu/maxmultimin.c:82-119) ask for at the same time.  The nb factorisations (with their inverse
 * rows) run in lock-step; outputs as gpemu_loglik_grad per element (grad: nb rows of nthetas-1),
 * status[b] = GPEMU_OK / GPEMU_ERR_NOT_PD / GPEMU_ERR_REGRESSION.  Workspace nb*(2N+64)*N*8 bytes. */
int gpemu_loglik_grad_batch(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas,
                            double *neg_loglik, double *sigma2, double *beta, double *grad,
                            int *info, int *status);
/* the same in two halves, like gpemu_loglik_batch_enqueue / _collect[_back]: enqueue puts the whole value+gradient
 * batch on the context's stream (staging, factorisation with inverse rows, C^-1 = U U^T, the gradient reductions, one
 * small copy into the pinned result ring) and returns without waiting -- no host synchronisation inside; collect waits
 * for THAT batch only and finishes on the host (the nreg x nreg solve and the reference's scalings, maxmultimin.c:
 * 503-535).  The ring is shared with the likelihood batches (GPEMU_RESULT_RING entries, `back` counts batches of
 * either kind; collecting a batch with the entry of the other kind is GPEMU_ERR_STATE).  A restart pool keeps two
 * contexts busy this way while its host threads do their BFGS arithmetic (estimate_threaded.c:172-188 keeps every
 * core busy; here: the device).  gpemu_loglik_grad_batch, gpemu_loglik_grad and gpemu_grad are enqueue + collect. */
int gpemu_loglik_grad_batch_enqueue(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas);
int gpemu_loglik_grad_batch_collect(gpemu_ctx *ctx, int nb, double *neg_loglik, double *sigma2, double *beta,
                                    double *grad, int *info, int *status);
int gpemu_loglik_grad_batch_collect_back(gpemu_ctx *ctx, int back, int nb, double *neg_loglik, double *sigma2,
                                         double *beta, double *grad, int *info, int *status);

/* ---- a14/a15: chol_inverse_cov_matrix + alloc_emulator_struct -------
 * (libEmu/emulate-fns.c:275-299, emulator_struct.c:13-37)
 * Factorises C(thetas) once and keeps L^-1, C^-1 [y|H], beta and
 * (H^T C^-1 H)^-1 resident in HBM.  beta_out[nreg] optional. */
int gpemu_predict_setup(gpemu_ctx *ctx, const double *thetas, int nthetas, double *beta_out, int *info);
/* alloc_multi_emulator (multivar_support.c:30-52: alloc_emulator_struct for each of the nr PCA components of a multi-output
 * model) as ONE lock-step batch: ctxs[0 .. n-1] hold the same design, covariance function, regression order and modes on the
 * same device and a training vector of their own each (gpemu_set_model / gpemu_set_training); component c is factored at
 * thetas[c * nthetas ..] with its inverse rows beside the others (one launch sequence for all, in ctxs[0]'s workspace) and
 * ctxs[c] receives the prediction state gpemu_predict_setup(ctxs[c], ...) would have given it, bit for bit.  beta_out
 * (n x nreg), info (n, 1-based failed pivot or 0) and status (n, GPEMU_OK / GPEMU_ERR_NOT_PD / GPEMU_ERR_REGRESSION per
 * component) are optional; the return value is the first failure (contexts of failed components are left without a set-up).
 * GPEMU_ERR_STATE, before any context is touched, while a host-buffer prediction batch is pending on one of the contexts
 * (collect it first); so are the other refusals that look at the contexts (a context without a model, listed twice, or of
 * another device, design, covariance function, order or mode): every context, those listed before the offending one too,
 * keeps its set-up, its joint factor and everything else.  gpemu_predict_setup itself does not refuse then: the pending batch was computed on the state it was
 * enqueued under and stays collectable with those bits. */
int gpemu_predict_setup_batch(gpemu_ctx *const *ctxs, int n, const double *thetas, int nthetas, double *beta_out, int *info,
                              int *status);
/* Pays what a process pays once -- the HIP runtime's start, the loading of this library's device code, its tables -- on a
 * throw-away context with a 64-point model, so that a caller can do it on a thread of its own while it is still reading its
 * input (interactive_mode: the snapshot).  Returns GPEMU_OK or the first error (GPEMU_ERR_NO_DEVICE ...). */
int gpemu_warm_start(int device);
/* optional: explicit C^-1 (N*N, both triangles) for emulator_struct.cinverse.  Reads the factorisation behind the set-up; on a
 * context set up as a later component of gpemu_predict_setup_batch, whose factorisation ran in ctxs[0]'s workspace, the first
 * call (of this entry, gpemu_sens_post[_dev] or gpemu_sens_pairs_post[_dev]) after the set-up factors that component again in
 * the context's own workspace, same thetas, same bits.  Either way nothing of the set-up changes: the prediction state, a
 * resident joint factor, a pending batch, the design block of gpemu_design_gain and the target store stay as they are.  That one
 * factorisation on a later component does take a slot of the context's result ring, as a gpemu_loglik would:
 * gpemu_loglik[_grad]_batch_collect_back reaches one batch less far back across it. */
int gpemu_get_cinverse(gpemu_ctx *ctx, double *cinv_out);

/* ---- a19: emulate_point, batched (emulator_struct.c:124-143) --------
 * mean[q], var[q] for M query rows xq[M*d].  Host buffers. */
int gpemu_predict_batch(gpemu_ctx *ctx, int npoints, const double *xq, double *mean, double *var);
/* the same in two halves: enqueue stages the queries through pinned memory and returns at once (the device work
 * runs on the context's stream), collect waits and copies the M means/variances out.  Different contexts -- the PCA
 * components of a multi-output emulator (multivar_support.c:103-157) -- work on their batches concurrently.
 * The one-batch-per-context rule, for this pair and the enqueue / collect pairs of gpemu_predict_mean, _mean_grad and
 * _var_grad below, which share its staging: a context has at most ONE batch pending, of whichever kind (an enqueue of any
 * kind while one is pending: GPEMU_ERR_STATE).  Only the collect of the batch's own kind takes it, with the npoints it was
 * enqueued with and the outputs that kind requires.  A refused collect -- another kind's or another npoints
 * (GPEMU_ERR_STATE), a required output NULL (GPEMU_ERR_ARG) -- leaves the batch pending.  gpemu_set_model drops it. */
int gpemu_predict_batch_enqueue(gpemu_ctx *ctx, int npoints, const double *xq /* M*d host */);
int gpemu_predict_batch_collect(gpemu_ctx *ctx, int npoints, double *mean, double *var);
/* same with query / result buffers already resident in HBM (device pointers) */
int gpemu_predict_batch_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev,
                            double *mean_dev, double *var_dev);

/* ---- the mean alone: makeEmulatedMean (emulator.c:672-704) over makeKVector_fnptr's clamped k-vector (:578-593) ----
 * mean[q] = h(x*_q)^T beta + sum_i k(x_i, x*_q) gamma_i,  gamma = C^-1 (y - H beta), for M query rows xq[M*d]: N kernel
 * evaluations and N multiply-adds per query, no product with L^-1 (that is the variance's).  The k values are the ones the
 * k-vectors of gpemu_predict_batch hold (same covariance code, nugget rule and < 1e-10 -> 0 clamp), used on chip: no k-vector
 * is written, the batch buffers of gpemu_predict_batch are neither touched nor allocated.  The value agrees with
 * gpemu_predict_batch's mean to rounding, NOT bit for bit: the sum over the design runs in another order.  That order is the
 * same for a query whatever else the call holds: two calls, a query alone or among others, any entry below -- same bits.
 * Any M (blocks of 16 384 internally).  GPEMU_ERR_STATE without a prediction set-up (gpemu_predict_setup or
 * gpemu_predict_setup_batch); GPEMU_ERR_ARG on a NULL pointer or npoints < 1.  The enqueue / collect pair follows the
 * one-batch-per-context rule stated at gpemu_predict_batch_enqueue. */
int gpemu_predict_mean(gpemu_ctx *ctx, int npoints, const double *xq, double *mean);
int gpemu_predict_mean_enqueue(gpemu_ctx *ctx, int npoints, const double *xq /* M*d host */);
int gpemu_predict_mean_collect(gpemu_ctx *ctx, int npoints, double *mean);
/* device pointers: only enqueues on the context's stream, no host synchronisation (the first call sizes the scratch) */
int gpemu_predict_mean_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, double *mean_dev);

/* ---- the mean and its gradient with respect to the query point ----
 * grad[q*d + j] = d mean(x*_q) / d x*_j of the function gpemu_predict_mean evaluates: with D_j = x*_j - x_ij,
 *   d k(x_i, x*) / d x*_j = -g_i s_j D_j      pow-exp  s_j = exp(-2 theta_{2+j}), g_i = k_i before the nugget
 *                                             Matern 3/2  s_j = c^2 / rho^2, g_i = A exp(-u)          (c = 1.732050808)
 *                                             Matern 5/2  s_j = 1 / rho^2, g_i = A exp(-u) ((c^2 - 10/3) + (5/3) u)  (c = 2.236067978)
 * (u = c distance / rho), g_i = 0 where the k value, nugget included, falls under the < 1e-10 -> 0 clamp, plus the regression
 * term sum_a beta_a dh_a/dx_j.  One fused sweep: the on-chip k tile is multiplied as weights with gamma_i [1, x_i - mid] on
 * the matrix unit; nothing of size M x N is stored, the batch buffers of gpemu_predict_batch are neither touched nor
 * allocated, the scratch is this entry's own.  mean (M values, may be NULL) agrees with gpemu_predict_mean to rounding, not
 * bit for bit.  A query's bits do not depend on the rest of the call or on the entry used.  Sizes, errors and the
 * enqueue / collect rule (the one stated at gpemu_predict_batch_enqueue) are those of gpemu_predict_mean. */
int gpemu_predict_mean_grad(gpemu_ctx *ctx, int npoints, const double *xq, double *mean /* M, may be NULL */, double *grad /* M*d row-major */);
int gpemu_predict_mean_grad_enqueue(gpemu_ctx *ctx, int npoints, const double *xq /* M*d host */);
int gpemu_predict_mean_grad_collect(gpemu_ctx *ctx, int npoints, double *mean /* may be NULL */, double *grad);
/* device pointers: only enqueues on the context's stream (the first call sizes the scratch) */
int gpemu_predict_mean_grad_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, double *mean_dev /* may be NULL */, double *grad_dev);

/* ---- mean, variance and the variance's gradient with respect to the query point ----
 * grad[q*d + j] = d var(x*_q) / d x*_j of the variance gpemu_predict_batch evaluates, var = kappa - |u|^2 + r^T Q r with
 * u = L^-1 k, r = h(x*) - W^T k, W = C^-1 H (kappa is constant: the nugget's add is constant on its box).  With the weights g_i
 * and constants s_j of gpemu_predict_mean_grad (g_i = 0 where the k value falls under the clamp), x' = x - mid:
 *   a = L^-T u + W (Q r)                                  one N-vector per query: a second N^2 product
 *   T_0 = sum_i a_i g_i,  T_j = sum_i a_i g_i x'_ij
 *   d var / d x*_j = 2 s_j ((x*_j - mid_j) T_0 - T_j) + 2 sum_a (Q r)_a dh_a/dx_j
 * Cost: two triangular products of M N^2 flops each (gpemu_predict_batch runs one) and one fused sweep.  Unlike the mean
 * sweeps this entry uses the batch buffers of gpemu_predict_batch (k-vectors and products, 8 M' (2 Np + 64) bytes for blocks of
 * M' <= 16384 queries), and the first call after a set-up makes a transposed copy of L^-1 with gamma and W: 8 Np (Np + 64)
 * bytes (0.54 GB at N = 8192), kept until the model is freed and rebuilt after every gpemu_predict_setup[_batch],
 * gpemu_set_model or gpemu_set_training.  Callers that never ask for this gradient allocate nothing for it.
 * mean and var (M values each, either may be NULL) agree with gpemu_predict_batch to rounding, not bit for bit.  Two
 * identical calls return the same bits; the host, _dev and enqueue / collect entries return the same bits.  Few queries take
 * the same kernels on one 64-row tile: there is no fast path for them.  Where the variance rounds to <= 0 the gradient is
 * still that of the expression above.
 * Errors are those of gpemu_predict_mean_grad (grad required; mean, var optional); the enqueue / collect pair follows the
 * one-batch-per-context rule stated at gpemu_predict_batch_enqueue. */
int gpemu_predict_var_grad(gpemu_ctx *ctx, int npoints, const double *xq, double *mean /* M, may be NULL */, double *var /* M, may be NULL */,
                           double *grad /* M*d row-major */);
int gpemu_predict_var_grad_enqueue(gpemu_ctx *ctx, int npoints, const double *xq /* M*d host */);
int gpemu_predict_var_grad_collect(gpemu_ctx *ctx, int npoints, double *mean /* may be NULL */, double *var /* may be NULL */, double *grad);
/* device pointers: only enqueues on the context's stream (the first call sizes the scratch and makes the transposed copy) */
int gpemu_predict_var_grad_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, double *mean_dev /* may be NULL */,
                               double *var_dev /* may be NULL */, double *grad_dev);

/* ---- joint posterior covariance between the query points of one call ----
 * cov[p*M + q] = Sigma_pq, the covariance between the emulator's errors at x*_p and x*_q (the "full predictive covariance"):
 *   Sigma_pq = c(x*_p, x*_q) - u_p . u_q + r_p^T Q r_q,   u_p = L^-1 k_p,  r_p = h(x*_p) - W^T k_p,
 * k_p the clamped k-vector of gpemu_predict_batch, c(.,.) the covariance function as gpemu_cov_matrix evaluates it on two
 * design rows: not clamped, with the reference's nugget rule (the nugget is added when every coordinate differs by less than
 * 1e-10, pow-exp, or 1e-16, Matern), GPEMU_MODE_MATERN_LOG honoured.  So Sigma_pp is gpemu_predict_batch's variance to
 * rounding; two identical query rows give identical rows and columns (Sigma is then singular, as the reference's C is for a
 * duplicated design row); Sigma is symmetric bit for bit (the upper triangle is a copy of the lower) and positive
 * semi-definite up to rounding.  mean (M values, may be NULL) agrees with gpemu_predict_batch to rounding.
 * Cost: the prediction sweep's M N^2 flops plus M^2 N for the symmetric product, 8 M^2 bytes of result; few queries take the
 * same kernels on one 64-row tile.  1 <= npoints <= 16384 (one block: 2 GB of result at the top); a larger npoints, a NULL
 * xq or cov: GPEMU_ERR_ARG before anything is allocated or launched.  GPEMU_ERR_STATE without a prediction set-up, and from
 * the host-buffer entry while a host-buffer batch of any kind is pending on the context (it stages through the same buffers;
 * the pending batch stays collectable).  Regression limits as for gpemu_predict_var_grad.  No enqueue / collect pair: the
 * result is M^2 numbers, not M.  The host-buffer entry keeps its 8 M^2-byte device copy until the model is freed.
 * Two identical calls return the same bits; the host and _dev entries and a context set up by gpemu_predict_setup_batch
 * return the same bits; no atomics.  The entry uses the batch buffers of gpemu_predict_batch and leaves nothing the other
 * prediction entries read. */
int gpemu_predict_cov(gpemu_ctx *ctx, int npoints, const double *xq /* M*d host */, double *mean /* M, may be NULL */,
                      double *cov /* M*M row-major, both triangles */);
/* device pointers: only enqueues on the context's stream (the first call sizes the scratch) */
int gpemu_predict_cov_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, double *mean_dev /* may be NULL */,
                          double *cov_dev /* M*M */);

/* ---- hold-out validation and joint draws at the query points of one call ----
 * S = Sigma + diag(noise), Sigma the joint covariance gpemu_predict_cov returns for the same queries (noise = NULL: none),
 * is built and factored on the device, S = L_S L_S^T (lower Cholesky factor, the factorisation of the likelihood), and never
 * leaves it.  With nobs rows of observations at the query points, yobs[a*M + p] (0 <= nobs <= 64):
 *   werr[a*M + .] = L_S^-1 (yobs_a - mean)     the decorrelated ("Cholesky") errors: independent N(0, 1) under the model
 *   maha[a]       = |werr_a|^2                  the squared Mahalanobis distance (yobs_a - mean)^T S^-1 (yobs_a - mean)
 *   logdet        = 2 sum_p log (L_S)_pp        log det S
 *   logpdf[a]     = -1/2 (maha[a] + logdet + M log 2 pi)     the joint log predictive density of row a
 *   var[p]        = S_pp as factored: gpemu_predict_batch's variance to rounding, plus noise_p
 * mean as gpemu_predict_cov returns it.  Every output may be NULL; yobs is NULL iff nobs = 0.
 * A successful call leaves {M, L_S, mean} resident in the context: gpemu_predict_joint_draw then returns, for ndraw rows of
 * standard normals z[s*M + .] supplied by the caller (any ndraw >= 1, blocks of 1024 internally),
 *   out[s*M + .] = mean + L_S z_s              a joint draw from N(mean, S)
 * so a draw with z = werr_a returns yobs_a.  The factor stays until the next factor call, gpemu_predict_joint_release,
 * gpemu_set_model, gpemu_set_training, gpemu_set_mode with other flags or gpemu_predict_setup[_batch]; it takes
 * 8 (M' + 64) M' bytes, M' = M rounded up to 64 (2.2 GB at M = 16384), which gpemu_predict_joint_release gives back.
 * Cost: gpemu_predict_cov's sweep and product (M N^2 + M^2 N flops, no mirror) plus M^3 / 3 for the factorisation of ONE
 * matrix; a block of draws is one triangular product of ndraw M^2 flops.  Few queries take the same kernels on one 64-row tile.
 * Failure: S is not positive definite to working precision -- coinciding query points without noise, or a negative
 * Sigma_pp + noise_p (the sign of noise is NOT checked: the device-pointer entry could not, so neither does): the host entry
 * returns GPEMU_ERR_NOT_PD with *info = the 1-based row of the failed pivot, mean and var valid, werr, maha, logdet and
 * logpdf NaN, and no factor is left (a draw then returns GPEMU_ERR_STATE).  *info = 0 otherwise.
 * Errors: GPEMU_ERR_ARG, before anything is allocated or launched, for a NULL ctx, xq or info, npoints outside 1 .. 16384, nobs
 * outside 0 .. 64, yobs NULL with nobs > 0, a NULL z or out, ndraw < 1; GPEMU_ERR_STATE without a prediction set-up, for a
 * draw without a resident factor, and from the two host-buffer entries while a host-buffer prediction batch is pending, as
 * for gpemu_predict_cov (the factor entry stages the queries through the same buffers; the batch stays collectable).
 * Two identical calls return the same bits; the host and _dev entries and a context set up by gpemu_predict_setup_batch return
 * the same bits; no atomics beyond the factorisation's info word.  The factor entry uses the batch buffers of
 * gpemu_predict_batch as gpemu_predict_cov does and leaves nothing the other prediction entries read. */
int gpemu_predict_joint_factor(gpemu_ctx *ctx, int npoints, const double *xq /* M*d host */, const double *noise /* M or NULL */,
                               int nobs, const double *yobs /* nobs*M rows, NULL iff nobs == 0 */,
                               double *mean /* M, may be NULL */, double *var /* M, may be NULL: the diagonal of S as factored */,
                               double *werr /* nobs*M, may be NULL */, double *maha /* nobs, may be NULL */,
                               double *logdet /* may be NULL */, double *logpdf /* nobs, may be NULL */, int *info);
/* device pointers: only enqueues on the context's stream (the first call sizes the buffers).  stat_dev (may be NULL): 1 + nobs
 * doubles, logdet then maha[0 .. nobs).  info_dev (required): one int, a value >= 0x7f7f7f7f for "no failed pivot", otherwise the
 * 1-based row; it is the caller's to read -- this entry cannot know about a failed pivot and marks the factor resident either
 * way.  A draw from a factor whose pivot failed returns unspecified numbers, reading inside the context's buffers only. */
int gpemu_predict_joint_factor_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, const double *noise_dev /* may be NULL */,
                                   int nobs, const double *yobs_dev, double *mean_dev /* may be NULL */, double *var_dev /* may be NULL */,
                                   double *werr_dev /* may be NULL */, double *stat_dev /* 1 + nobs, may be NULL */, int *info_dev);
int gpemu_predict_joint_draw(gpemu_ctx *ctx, int ndraw, const double *z /* ndraw*M host */, double *out /* ndraw*M host */);
/* device pointers: only enqueues on the context's stream.  out_dev may be z_dev itself (each element is read before it is written). */
int gpemu_predict_joint_draw_dev(gpemu_ctx *ctx, int ndraw, const double *z_dev, double *out_dev);
/* drops the resident factor and frees every buffer of the joint entries (waits for the context's stream) */
int gpemu_predict_joint_release(gpemu_ctx *ctx);

/* ---- leave-one-out validation of a trained emulator -----------------
 * mean[i], var[i] for every training point i: what removing point i, alloc_emulator_struct on the other N - 1 points at
 * the same thetas and emulate_point at x_i return (GLS beta re-estimated, variance with the regression term and kappa
 * including the nugget: emulator.c:672-785, emulator_struct.c:124-143), from the state gpemu_predict_setup[_batch] left
 * in HBM, in closed form (Dubrule 1983, universal kriging).  With P = C^-1 - W Q W^T, W = C^-1 H, Q = (H^T C^-1 H)^-1:
 *   P_ii = sum_{k >= i} (L^-1)_ki^2 - w_i^T Q w_i,   var_i = 1 / P_ii,   mean_i = y_i - gamma_i / P_ii
 * One pass over the lower triangle of L^-1 (8 N (N+1) / 2 bytes) instead of N factorisations.
 * One difference from the refit: the closed form works on the matrix C, whose elements are not clamped, while the refit's
 * k-vector (makeKVector_fnptr, emulator.c:588-590) zeroes entries below 1e-10.  Where no off-diagonal element of C is
 * below 1e-10 the two agree to rounding; where some are, they differ by at most the effect of those entries.
 * GPEMU_ERR_STATE without a valid prediction set-up; GPEMU_ERR_ARG when N <= nreg + 1 (no degrees of freedom are left with
 * one point removed) or an output is NULL.  Two calls on the same state return the same bits. */
int gpemu_loo(gpemu_ctx *ctx, double *mean /* N host */, double *var /* N host */);
/* the same with result buffers in HBM (device pointers): only enqueues on the context's stream, no host sync */
int gpemu_loo_dev(gpemu_ctx *ctx, double *mean_dev, double *var_dev);

/* ---- K-fold / leave-group-out validation of a trained emulator -----------------
 * group[i] in 0 .. ngroups-1 names the group training point i is left out with, -1: never left out.  For every group B (b
 * points, taken in ascending design index): what removing ALL of B, alloc_emulator_struct on the other N - b points at the
 * same thetas and gpemu_predict_cov at x_B return -- GLS beta re-estimated, the variance with the regression term, kappa
 * with the nugget, as gpemu_loo stands for with one point -- from the state gpemu_predict_setup[_batch] left in HBM, by the
 * block form of gpemu_loo's closed form.  With P = C^-1 - W Q W^T and gamma = P y:
 *   (P_BB)_ij = sum_k (L^-1)_ki (L^-1)_kj - w_i^T Q w_j        P_BB = R R^T (lower Cholesky, the likelihood's factorisation)
 *   cov_B     = P_BB^-1           mean_B = y_B - cov_B gamma_B          var_i = (cov_B)_ii = sum_k (R^-1)_ki^2
 *   werr_B    = R^-1 gamma_B = R^T (y_B - mean_B)      the decorrelated errors of the group: independent N(0, 1) under the model
 *   maha[g]   = |werr_B|^2 = (y_B - mean_B)^T cov_B^-1 (y_B - mean_B)
 *   logdet[g] = log det cov_B = -2 sum_i log R_ii       logpdf[g] = -1/2 (maha[g] + logdet[g] + b log 2 pi)
 * With b = 1 this is gpemu_loo.  werr whitens with the UPPER factor R^-T of cov_B (cov_B = R^-T R^-1): werr_i depends on the
 * errors of the group's members k >= i.  gpemu_predict_joint_factor's werr uses the lower factor of its S, so for the same
 * points the two are different vectors of the same norm.
 * mean, var, werr: N each, in design order, NaN where group[i] = -1; maha, logdet, logpdf, info: ngroups each.
 * The clamp remark of gpemu_loo holds unchanged: the closed form reads C, which is not clamped; a refit's k-vector is.
 * How it runs: chunks of at most GPEMU_MAX_BATCH groups, every group of the CALL padded to bp = the largest group rounded up
 * to 64; per chunk of nbc groups a gather of the members' columns of L^-1, one batched product, a staging pass, ONE lock-step
 * factorisation with inverse rows of the nbc matrices, and a finishing pass, all on the context's stream.  Memory per chunk:
 * 8 nbc bp (Np + 2 bp + 64) bytes (Np = N rounded up to 64) plus 8 nbc (bp / 64 + 2) bytes of partial sums and the index
 * tables (4 (2 N + 2 ngroups) bytes, device and pinned); nbc = the most groups, at most 64 and at least one, that keep the
 * formula within 2 GiB (fixed, so the chunking depends on the call alone).  gpemu_lgo_release gives the buffers back (waits
 * for the stream); gpemu_set_model and the end of the context free them too.
 * A group whose P_BB is not positive definite to working precision: info[g] = the 1-based position of the failed pivot within
 * the group (0 otherwise), NaN in all its outputs; the other groups stay valid, and the host entry returns GPEMU_ERR_NOT_PD.
 * Errors: GPEMU_ERR_ARG for a NULL ctx, group, mean, var or info and for ngroups < 1, whatever the context's state;
 * GPEMU_ERR_STATE without a valid prediction set-up; then GPEMU_ERR_ARG, before anything is allocated or launched, for
 * ngroups > N, a label outside -1 .. ngroups-1, a label without members, a largest group b_max with N - b_max <= nreg (no
 * degrees of freedom left: gpemu_loo's rule), bp > 16384.
 * Two identical calls return the same bits; the host and _dev entries and a context set up by gpemu_predict_setup_batch return
 * the same bits.  A group's bits may depend on the other groups of the call (the common padded size does).  No atomics beyond
 * the factorisation's info words, no workgroup waits for another.  The entry works in buffers of its own: it leaves nothing
 * another entry reads, a pending host-buffer prediction batch stays collectable, gpemu_get_cinverse keeps working. */
int gpemu_lgo(gpemu_ctx *ctx, int ngroups, const int *group /* N host */, double *mean /* N */, double *var /* N */,
              double *werr /* N, may be NULL */, double *maha /* ngroups, may be NULL */, double *logdet /* ngroups, may be NULL */,
              double *logpdf /* ngroups, may be NULL */, int *info /* ngroups */);
/* result buffers in HBM (device pointers), group still a HOST array (sizes and chunking are decided on the host): only
 * enqueues on the context's stream.  stat_dev: maha[0 .. ngroups), then logdet[0 .. ngroups), then logpdf[0 .. ngroups);
 * info_dev[g]: 0 or the 1-based position, already decoded.  The index tables go up through a pinned buffer of the context:
 * a call first waits (on the host) until the previous call's upload out of that buffer has executed -- not for its kernels. */
int gpemu_lgo_dev(gpemu_ctx *ctx, int ngroups, const int *group /* N HOST */, double *mean_dev, double *var_dev,
                  double *werr_dev /* may be NULL */, double *stat_dev /* 3*ngroups, may be NULL */, int *info_dev /* ngroups */);
/* frees every buffer of the two entries above (waits for the context's stream) */
int gpemu_lgo_release(gpemu_ctx *ctx);

/* ---- main effects and Sobol indices of the posterior mean, in closed form -----------------
 * Stands in for the reference's sensitivity analysis in R (src/libSA/sa-fns.R: the Oakley-O'Hagan integrals of a
 * squared-exponential emulator with a (1, x) regression).  The input measure is independent per coordinate and, by default,
 * a BOX -- uniform inputs on [lo_l, hi_l], the caller's box, which may be narrower than the design or leave design points
 * outside.  The reference integrates against a GAUSSIAN input measure: gpemu_sens_set_measure (below, after gpemu_sens_joint)
 * makes any coordinate Gaussian, and lo_l / hi_l then mean its mean and standard deviation in every entry of this family.
 * This is the plug-in analysis of the posterior mean; the
 * emulator-uncertainty terms of Oakley-O'Hagan are gpemu_sens_post's and gpemu_sens_main_var's, below.
 * The function analysed is the one gpemu_predict_mean evaluates, for the power-exponential covariance, without the k-vector
 * clamp:   m(x) = beta_0 + sum_l q_l(x_l) + A sum_i gamma_i prod_l k_l(x_il, x_l),   q_l(x) = sum_{p=1..order} beta_{p,l} x^p,
 * k_l(a, x) = exp(-s_l (x - a)^2 / 2), s_l = exp(-2 theta_{2+l}), A the amplitude of the k-vector.  The nugget rule acts on a
 * set of measure zero and drops out; the clamp does not (the remark at gpemu_loo): the closed form integrates the unclamped
 * kernel, the two functions differ by at most sum_i |gamma_i| 1e-10.
 * The kernel is a product of one-dimensional Gaussians and the regression basis is additive in the coordinates, so every
 * conditional expectation m_u = E[m | x_u] factorises into one-dimensional integrals with an erf closed form.  For two
 * contexts a and b on the SAME design (lengths s and t, weights gamma and gamma', amplitudes A and A'; b may be a):
 *   e0[0], e0[1]   E[m^a], E[m^b]
 *   cov_all        Cov(m^a, m^b)                                with b = a: V, the total variance
 *   cov_first[j]   Cov(m^a_{j}, m^b_{j})                        with b = a: V_j, the first-order variance of coordinate j
 *   cov_rest[j]    Cov(m^a_{-j}, m^b_{-j})  (all but j known)   with b = a: V - cov_rest[j] = VT_j, the total-effect variance
 * The cross case is what a multi-output emulator needs: its PCA components are not independent under the input measure.
 * gpemu_sens_main returns E0 and the main-effect curves main[j*ngrid + g] = E[m | x_j = grid[j*ngrid + g]].
 * How it runs, three launches on a's stream: the per-point integrals of both contexts (five N x d tables each: I, J^1, J^2, J^3
 * and the leave-one-out products of I); the full N x N square of pair terms in 64 x 64 tiles, 2 d + 1 partial sums per tile
 * (2 N^2 d erf evaluations: bound by vector fp64); the finish, which adds the partials in a fixed order and assembles the
 * polynomial parts, E0 removed from the constant term before any second moment is formed.  An erf difference whose arguments
 * have one sign is taken as an erfc difference, and leave-one-out products come from prefix and suffix products, never from
 * a division.  d <= 16 keeps its per-coordinate values in registers; a larger d (any up to GPEMU_MAX_PARAMS) takes the same
 * loop rolled, with them in private memory: slower.  Memory: 8 (10 N d + ceil(N / 64)^2 (2 d + 1)) bytes.
 * No atomics, no workgroup waits for another.  Two identical calls return the same bits, and so do the host and _dev entries
 * and a context set up by gpemu_predict_setup_batch.  The _dev entry only enqueues (lo and hi are HOST arrays: they travel as
 * kernel arguments); with b != a it orders a's stream behind b's pending work, and b's stream behind the call, with events:
 * no host synchronisation.  The entries work in buffers of their own, in a: they leave nothing another entry reads, a pending
 * prediction batch stays collectable; gpemu_sens_release gives the buffers back (waits for the stream), gpemu_set_model and
 * the end of the context free them too.
 * Errors, before anything is allocated or launched: GPEMU_ERR_ARG for a NULL pointer and ngrid < 1, whatever the state;
 * GPEMU_ERR_STATE without a prediction set-up on either context; then GPEMU_ERR_ARG for a Matern model (the closed form
 * exists for the power-exponential covariance only), contexts on different devices, contexts whose designs differ in N, d
 * or any coordinate (the host copies are compared) or whose regression orders differ, a non-finite bound or hi_l <= lo_l. */
int gpemu_sens_cov(gpemu_ctx *a, gpemu_ctx *b /* may be a */, const double *lo, const double *hi /* d each, host */,
                   double *e0 /* 2: E0 of a, of b */, double *cov_all, double *cov_first /* d */, double *cov_rest /* d */);
int gpemu_sens_cov_dev(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi /* HOST */,
                       double *out_dev /* 3 + 2 d: e0a, e0b, cov_all, first[d], rest[d] */);
int gpemu_sens_main(gpemu_ctx *ctx, const double *lo, const double *hi, int ngrid, const double *grid /* d*ngrid host: row j = values of x_j */,
                    double *e0, double *main /* d*ngrid: E[m | x_j = grid[j][g]] */);
int gpemu_sens_release(gpemu_ctx *ctx);

/* ---- emulator uncertainty of the main effects and Sobol indices, in closed form -----------------
 * The entries above analyse the posterior MEAN.  These add what the emulator does not know: the terms the reference's
 * src/libSA/trivial-test-2.R evaluates per point of a main-effect curve and plots as a confidence band.  f is the posterior
 * process with mean m and covariance (no k-vector clamp, and no nugget anywhere: it is jitter, not part of the function)
 *   c*(x, x') = c(x, x') - k(x)^T C^-1 k(x') + r(x)^T Q r(x'),   r(x) = h(x) - W^T k(x),  W = C^-1 H,  Q = (H^T C^-1 H)^-1.
 * For a set u of coordinates, S_u = E_{x_u} Var*[E[f | x_u]]: c* integrated over the box with the coordinates of u shared
 * between x and x' and the others independent.  gpemu_sens_post returns
 *   s_none       S for u empty: Var*[E0], the posterior variance of the overall mean
 *   s_all        S for u = all: the box average of the posterior variance of f (the IMSE of the design); the box average of
 *                gpemu_predict_batch's variance minus the nugget, up to the clamp
 *   s_first[j]   S for u = {j}          s_rest[j]   S for u = all but j
 * with s_none <= s_first[j], s_rest[j] <= s_all (Jensen).  With V, V_j = cov_first[j], VT_j = V - cov_rest[j] of
 * gpemu_sens_cov(ctx, ctx), the posterior expectations of the variances of f itself are
 *   E*[V] = V + s_all - s_none,   E*[V_j] = V_j + s_first[j] - s_none,   E*[VT_j] = VT_j + s_all - s_rest[j].
 * One context: the PCA components of a multi-output emulator are independent a posteriori, there is no cross case.
 * gpemu_sens_main_var returns, per grid value, var[j*ngrid + g] = Var*[E[f | x_j = grid[j*ngrid + g]]], the curve itself
 * (main, as gpemu_sens_main's to rounding) and var_e0 = Var*[E0] (s_none to rounding).
 * How gpemu_sens_post runs, on the context's stream: the per-point tables of gpemu_sens_cov; the corner C^-1 = U U^T that
 * gpemu_get_cinverse caches (built once per set-up; 2 N^3 / 3 flops the first time, read only); a launch that writes G = W Q
 * and P = C^-1 - G W^T on the lower 64 x 64 tiles; the pair sweep of gpemu_sens_cov over the LOWER tiles, every pair term
 * weighted by its element of P in place of gamma_i gamma_i', 2 d + 2 partial sums per tile; the finish.  Memory: 8 (N'^2 +
 * N nreg + T') bytes besides the tables and the corner, N' = N rounded up to 64, T' = ceil(N/64) (ceil(N/64) + 1) / 2 (2 d + 2).
 * gpemu_sens_main_var: the tables, d ngrid + 1 rows T_i = A k_j(x_ij, x) Pex_j(i) into the prediction's k-vector buffer, the
 * prediction's product with [L^-1; gamma; W^T] (K never split), a finish with T for the k-vector and E[h | x_j = x] for h.
 * It uses the prediction batch buffers in stream order, as gpemu_predict_cov_dev does; a pending prediction batch stays
 * collectable.  No atomics, no workgroup waits for another; two calls return the same bits, so do the host and _dev entries and
 * a context set up by gpemu_predict_setup_batch (a later component of such a batch factors alone first, as for
 * gpemu_get_cinverse).  gpemu_sens_release frees these entries' buffers too.
 * Errors as for gpemu_sens_cov, before anything is allocated or launched: GPEMU_ERR_ARG for a NULL pointer (main and var_e0
 * may be NULL) and ngrid < 1; GPEMU_ERR_STATE without a prediction set-up; GPEMU_ERR_ARG for a Matern model, a non-finite
 * bound or hi_l <= lo_l. */
int gpemu_sens_post(gpemu_ctx *ctx, const double *lo, const double *hi /* d each, host */,
                    double *s_none, double *s_all, double *s_first /* d */, double *s_rest /* d */);
int gpemu_sens_post_dev(gpemu_ctx *ctx, const double *lo, const double *hi /* HOST */,
                        double *out_dev /* 2 + 2 d: s_none, s_all, first[d], rest[d] */);
int gpemu_sens_main_var(gpemu_ctx *ctx, const double *lo, const double *hi, int ngrid, const double *grid /* d*ngrid host */,
                        double *main /* d*ngrid, may be NULL */, double *var /* d*ngrid */, double *var_e0 /* may be NULL */);

/* ---- expected reduction of the IMSE by one more run, in closed form -----------------
 * s_all of gpemu_sens_post says whether more model runs are needed; these entries say where to put one.  Conditioning the
 * posterior process on a run at x* is a rank-one update of its covariance, so for each of npoints candidates
 *   gain(x*) = E_x[c*(x, x*)^2] / v(x*) = s_all(design) - s_all(design + {x*}),     hyper-parameters as they are,
 * with the conventions of the entries above (no k-vector clamp, no nugget rule inside c), the measure of the context
 * (gpemu_sens_set_measure; lo / hi as in the gpemu_sens_* family), and for k* = k(x*), h* = h(x*)
 *   u = L^-1 k*,  r = h* - W^T k*,  b = Q r,  a = L^-T u + W b,   c*(x, x*) = c(x, x*) - k(x)^T a + h(x)^T b,
 *   var = v(x*) = A - |u|^2 + r^T Q r + nugget      (the variance a new run at x* is observed with),
 *   num = A^2 prod_l II_l(x*, x*) - 2 A^2 sum_i a_i w_i + 2 A sum_al b_al HK*_al + A^2 a^T K a - 2 A sum_al b_al (a^T HK_al) + b^T Hm b,
 * K_ii' = prod_l II_l(x_i, x_i'), w_i = prod_l II_l(x_i, x*), HK_al,i = E[h_al(x) prod_l k_l(x_il, x_l)] (HK* the same at x*),
 * Hm = E[h h^T].  gain = num / var; where var rounds to <= 0 (nugget 0 on a design point) gain is 0; num and var (either may
 * be NULL) are returned as computed.  var is gpemu_predict_batch's variance up to the clamp.
 * How it runs, on the context's stream: the per-point tables of gpemu_sens_cov for the design; [K ; HK] over 64 x 64 tiles
 * and Hm, kept on the context (8 Np (Np + 64) bytes) and rebuilt when the set-up, the box or the kinds differ from the last
 * call's; then per block of up to 16 384 candidates the same tables for the candidates, the unclamped k rows, the prediction's
 * product with [L^-1; gamma; W^T] and the second triangular product of gpemu_predict_var_grad (its transposed copy of L^-1,
 * made on first use) for a, T = a [K | HK] (the third M N^2 product), a sweep over 64 candidates x 64 design points per
 * workgroup for sum_i a_i (T_i - 2 w_i) and a finish of one wave per candidate.  d <= 16 keeps the candidate's coordinates in
 * registers; a larger d takes the rolled form.  It uses the prediction batch buffers in stream order, as gpemu_predict_cov_dev
 * does; a pending prediction batch stays collectable.  Memory per block of mb candidates: 8 mb (2 Np + 10 d + 192 + ceil(N/64))
 * bytes of its own.  No atomics, no workgroup waits for another; two calls return the same bits, so do the host and _dev entries,
 * a candidate alone and in a batch, and a context set up by gpemu_predict_setup_batch.  gpemu_sens_release frees its buffers.
 * Errors, before anything is allocated or launched: GPEMU_ERR_ARG for a NULL ctx, lo, hi, xq or gain and npoints < 1, whatever
 * the state; GPEMU_ERR_STATE without a prediction set-up; then GPEMU_ERR_ARG for a Matern model, a non-finite bound, hi_l <= lo_l
 * or a Gaussian coordinate with sd <= 0.
 * Not built: the gradient of gain with respect to x* and any optimiser over it (greedy batches: gpemu_design_batch below);
 * Matern kernels in this closed form (gpemu_design_target_gain below takes them: its target is a point set); gain for a
 * target other than the IMSE or a point set (Sobol-index uncertainty); correlated Gaussian measures. */
int gpemu_design_gain(gpemu_ctx *ctx, const double *lo, const double *hi /* d each, host */, int npoints,
                      const double *xq /* npoints*d host */, double *gain /* npoints */, double *num /* npoints or NULL */,
                      double *var /* npoints or NULL */);
int gpemu_design_gain_dev(gpemu_ctx *ctx, const double *lo, const double *hi /* HOST */, int npoints, const double *xq_dev,
                          double *gain_dev, double *num_dev /* or NULL */, double *var_dev /* or NULL */);

/* ---- greedy batches of K runs: conditional IMSE gains, picks on the device -----------------
 * The top K candidates of gpemu_design_gain sit next to each other: the first run there removes most of what the others would
 * gain.  These entries pick nbatch of npoints candidates one after the other, each the arg-max of the gain CONDITIONAL on the
 * picks before it, without a refit.  With Sigma(q, s) = c*(x_q, x_s) and G(q, s) = E_x[c*(x, x_q) c*(x, x_s)] (both from the
 * rows a_q, T_q, w_q of the first pass and a handful of vectors of s; G(q, q) = num_q, Sigma(q, q) = var_q - nugget) the state
 * per candidate is lambda_q, mu_q in R^j after j picks, and a j x j matrix E shared by all candidates:
 *   v_S(q) = var_q - |lambda_q|^2,   num_S(q) = num_q - 2 lambda_q . mu_q + lambda_q^T E lambda_q,   gain_S(q) = num_S(q) / v_S(q)
 * (0 where v_S(q) rounds to <= 0); the pick s is the arg-max of sum_c weight_c gain_S,c(q) over the candidates not yet picked,
 * ties to the lowest index, NaN never preferred; then with rho = sqrt(v_S(s))
 *   lambda_q,new = (Sigma(q, s) - lambda_q . lambda_s) / rho,   mu_q,new = (G(q, s) - mu_q . lambda_s) / rho,
 *   E_i,new = (mu_s,i - (E lambda_s)_i) / rho,   E_new,new = num_S(s) / v_S(s).
 * A pick whose v_S rounds to <= 0 changes nothing (its lambda, mu and column of E are 0).  pick_gain[j] is the further drop of
 * the (weighted) IMSE by pick j: the sum of the first j equals s_all(design) - s_all(design + the first j picks), the hyper-
 * parameters as they are.  The contexts are the independent components of a multi-output emulator on one design (as
 * gpemu_sens_pairs requires of two contexts: same device, design, order and input measure); one run observes all of them, each
 * keeps its own state, and weight (NULL: all 1) weighs their gains.  Where fewer than nbatch candidates have a positive gain
 * the picks go on by the same rule (among equal gains the lowest index not yet picked).
 * Outputs: pick[j] the index of pick j, pick_gain[j] its weighted gain, pick_gain_ctx[j * nctx + c] (may be NULL) the
 * contexts' own, gain_first[q] (may be NULL) the weighted gain before any pick -- for one context and weight 1 the bits of
 * gpemu_design_gain -- and gain_last[q] (may be NULL) the weighted gain conditional on all nbatch picks, -inf for a picked q.
 * How it runs, per context on its own stream: one block of gpemu_design_gain_dev (its launches, its bits), a launch for the rows
 * of w; per pick a gather (the pick's a, w, fresh unclamped k rows, b, h, T^HK, HK*, Hm b, lambda, the new column of E), the
 * column kernel (the rows of a, T^K and w of every candidate streamed once for the four dots a_q . k_s, a_q . w_s, w_q . a_s,
 * T^K_q . a_s: 24 M' Np bytes, bandwidth-bound), and the update (one wave per candidate: the short terms, the new lambda and
 * mu, v_S, num_S and gain, the quadratic form carried forward in O(j)).  The arg-max is one launch on ctxs[0]'s stream, which
 * waits on the other streams by events; they wait on its event.  The host takes no part between picks.  No atomics, no
 * workgroup waits for another; every sum has one order: two calls return the same bits, so do the host and _dev entries, the
 * first j picks of a longer batch and a batch of j, and contexts set up by gpemu_predict_setup_batch.
 * Memory per context beyond gpemu_design_gain's: 8 M' Np bytes for w, 16 M nbatch for lambda and mu, 512 KiB for E,
 * 8 (3 Np + 1024 + 7 M) for the gather, the dots and the running state.  gpemu_sens_release frees it.
 * Limits: 1 <= npoints <= 16 384 (one block), 1 <= nbatch <= min(npoints, 256).
 * Errors, before anything is allocated or launched: GPEMU_ERR_ARG for a NULL ctxs, ctxs[c], lo, hi, xq, pick or pick_gain,
 * nctx < 1 and counts out of range, whatever the state; GPEMU_ERR_STATE for a context without a prediction set-up; then
 * GPEMU_ERR_ARG for a Matern model, a bad box, sd <= 0, differing designs, orders, measures or devices, a context listed
 * twice, a negative or non-finite weight.
 * Not built: more than one block of candidates; exchange or other non-greedy criteria; the gradient of the gain; Matern kernels. */
int gpemu_design_batch(gpemu_ctx *const *ctxs, int nctx, const double *weight /* nctx host, or NULL: all 1 */, const double *lo,
                       const double *hi /* d each, host */, int npoints, const double *xq /* npoints*d host */, int nbatch,
                       int *pick /* nbatch */, double *pick_gain /* nbatch: the weighted sum */,
                       double *pick_gain_ctx /* nbatch*nctx or NULL */, double *gain_first /* npoints or NULL */,
                       double *gain_last /* npoints or NULL */);
/* the same with xq, pick, pick_gain, pick_gain_ctx, gain_first and gain_last in device memory; the results are complete behind
 * ctxs[0]'s stream */
int gpemu_design_batch_dev(gpemu_ctx *const *ctxs, int nctx, const double *weight /* HOST */, const double *lo, const double *hi /* HOST */,
                           int npoints, const double *xq_dev, int nbatch, int *pick_dev, double *pick_gain_dev, double *pick_gain_ctx_dev,
                           double *gain_first_dev, double *gain_last_dev);

/* ---- gain over a weighted set of target points: variance drop where the posterior is -----------------
 * After a calibration the next run is wanted where the emulator's variance drops over the region the observations left
 * standing, not over the box.  That region is a weighted point set x_s, w_s >= 0, s = 1 .. S (chain samples of
 * gpemu_calib_sample, the points gpemu_calib_select kept, quadrature nodes); no integral has to exist in closed form, so
 * every covariance function is served.  With u = L^-1 k, r = h - W^T k (the quantities of gpemu_predict_cov) and
 *   c*(x_s, x*) = c(x_s, x*) - u_s . u_* + r_*^T Q r_s
 * for each of npoints candidates x*
 *   var  = c*(x*, x*) + nugget                (the variance a run at x* is observed with; gpemu_design_gain's var),
 *   num  = sum_s w_s c*(x_s, x*)^2,
 *   gain = num / var = sum_s w_s [v(x_s) - v_{+x*}(x_s)],      hyper-parameters as they are,
 * and the set entry returns v(x_s) = c*(x_s, x_s) (latent: no nugget) per target and target_var = sum_s w_s v(x_s), so that
 * 0 <= gain <= target_var.  Conventions of gpemu_design_gain, not of gpemu_predict_cov: no k-vector clamp, no nugget rule
 * inside c or k (a target or candidate on a design point, or on each other, gets the bare kernel value); var carries the
 * nugget once; where var rounds to <= 0 gain is 0; num and var (either may be NULL) are returned as computed.  The weights
 * are used as given (NULL: 1 / S each), not normalised.
 * How it runs, on the context's stream.  gpemu_design_target_set copies coordinates and weights into the context and builds
 * the resident store per block of up to 16 384 targets through the prediction batch buffers, as gpemu_design_gain_dev uses
 * them: the unclamped nugget-free k rows (the stored fill, mode 0), the product with [L^-1; gamma; W^T], the prediction's
 * finish for v, Q r per target; u (S' x Np), r and Q r are copied out, target_var is summed in one fixed order.  The store
 * belongs to one prediction set-up: after another gpemu_predict_setup the next gain call rebuilds it from the kept
 * coordinates.  gpemu_design_target_gain, per block of up to 16 384 candidates: the same chain (var as the prediction's finish
 * takes it), then per panel of target columns (GPEMU_TARGET_PANEL in the environment at gpemu_ctx_create, a multiple of 64,
 * default 2048) the full product P = U_q U_t^T on the GEMM, a sweep of one workgroup per 64 candidates x 64 targets (the tile
 * of P read as row pieces, c through the stored fill's tile function, r . Q r from LDS, w_s c*^2 reduced over the tile's 64
 * targets in a fixed order: one partial per candidate and target tile) and a finish that adds the partials in ascending tile
 * order to the running num and forms the quotient behind the last panel.  No atomics, no workgroup waits for another; the sum
 * over the targets has one order: two calls return the same bits, so do the host and _dev entries, a candidate alone and in
 * a batch, any panel width, and a context set up by gpemu_predict_setup_batch.  A pending prediction batch stays collectable.
 * Limits: 1 <= ntargets <= 65 536; npoints >= 1.  Memory: 8 S' (Np + 2 Rp + d + 2) bytes for the store (S' = ntargets rounded
 * up to 64), per block of mb candidates 8 mb (64 + panel + panel / 64 + 3) more; gpemu_design_target_release, gpemu_set_model
 * and gpemu_ctx_destroy free it.  The _set entries wait for the upload of the weights; everything else of the _dev entries is
 * only enqueued.
 * Errors, before anything is allocated or launched: GPEMU_ERR_ARG for a NULL ctx, xt, xq or gain, a count out of range, a
 * negative or non-finite weight, weights that sum to 0 and (host entries: device coordinates are not read) a non-finite
 * coordinate; then GPEMU_ERR_STATE without a prediction set-up, and for a gain call without targets.
 * Not built: greedy batches over a target set (they need the M x S matrix kept and a rank-one pass per pick); weights in
 * device memory; more than 65 536 targets; the gradient of the gain; targets drawn by the library itself. */
int gpemu_design_target_set(gpemu_ctx *ctx, int ntargets, const double *xt /* ntargets*d host */,
                            const double *weight /* ntargets host, or NULL: 1/ntargets each */, double *target_var /* 1, may be NULL */,
                            double *var_t /* ntargets, may be NULL */);
int gpemu_design_target_set_dev(gpemu_ctx *ctx, int ntargets, const double *xt_dev, const double *weight /* HOST or NULL */,
                                double *target_var_dev, double *var_t_dev);
int gpemu_design_target_gain(gpemu_ctx *ctx, int npoints, const double *xq /* npoints*d host */, double *gain /* npoints */,
                             double *num /* npoints or NULL */, double *var /* npoints or NULL */);
int gpemu_design_target_gain_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, double *gain_dev, double *num_dev /* or NULL */,
                                 double *var_dev /* or NULL */);
int gpemu_design_target_release(gpemu_ctx *ctx);

/* ---- second-order Sobol indices and interaction surfaces, in closed form -----------------
 * VT_j - V_j > 0 says that parameter j interacts with something; these entries say with which parameter, and what the
 * interaction looks like.  For u = {j, k} every conditional expectation still factorises into the one-dimensional integrals
 * above.  Pairs j < k are numbered p(j, k) = j (2 d - j - 1) / 2 + (k - j - 1), npairs = d (d - 1) / 2.
 * gpemu_sens_pairs returns cov_pair[p(j, k)] = Cov(E[m^a | x_j, x_k], E[m^b | x_j, x_k]) for two contexts on the same design
 * (b may be a).  With b = a this is V_jk; the interaction variance is V_jk - V_j - V_k (V_j = cov_first[j] of gpemu_sens_cov)
 * and the second-order index is that over V.  The cross case is what a multi-output emulator needs, as for gpemu_sens_cov.
 * gpemu_sens_pairs_post returns s_pair[p(j, k)] = S_u of gpemu_sens_post for u = {j, k}, s_none <= s_first[j], s_first[k] <=
 * s_pair <= s_all, and with it the posterior expectations
 *   E*[V_jk] = V_jk + s_pair - s_none,
 *   E*[V_jk - V_j - V_k] = V_jk - V_j - V_k + s_pair - s_first[j] - s_first[k] + s_none.
 * gpemu_sens_joint returns, for one pair j != k and npts points (xj[g], xk[g]), E0, the two-way surface
 * joint[g] = E[m | x_j = xj[g], x_k = xk[g]] and the interaction effect inter[g] = joint - main_j - main_k + E0.  The
 * regression basis is additive, so the polynomial parts of inter cancel exactly; it is summed as
 * A sum_i gamma_i [k_j k_k Pex2_jk - k_j Pex_j - k_k Pex_k + prod_l I_l](i), never as a difference of the large values.
 * How they run: the per-point tables of gpemu_sens_cov; a launch that writes the leave-two-out products
 * Pex2_jk(i) = prod_{l != j,k} I_l(i) of both contexts (prefix, running-middle and suffix products: O(d^2) per point, no
 * division); the pair sweep, 64 x 64 tiles of point pairs times blocks of 8 x 8 coordinates -- one launch for the blocks on
 * the diagonal (28 pairs, 8 one-dimensional integrals per pair of points), for d > 8 one more for the others (64 pairs, 16
 * integrals) -- which leaves npairs partial sums per tile; the finish.  gpemu_sens_pairs_post weights every pair term by its
 * element of P over the lower tiles, as gpemu_sens_post does (the same launch writes P and G).  gpemu_sens_joint: the tables,
 * then one workgroup per point.  Any d from 2 to GPEMU_MAX_PARAMS takes the same kernels, all sums in registers.
 * Memory, besides the tables of gpemu_sens_cov (and P, G and the corner for the post entry):
 * 8 (2 N npairs + ceil(N / 64)^2 npairs + npairs) bytes; gpemu_sens_joint 8 (2 N npairs + 4 npts).
 * No atomics, no workgroup waits for another, every sum has one order: two calls return the same bits, and so do the host and
 * _dev entries and a context set up by gpemu_predict_setup_batch.  The _dev entries only enqueue; with b != a the streams are
 * ordered by events as for gpemu_sens_cov_dev.  The buffers are the entries' own: a pending prediction batch stays
 * collectable; gpemu_sens_release, gpemu_set_model and the end of the context free them.
 * Errors, before anything is allocated or launched: GPEMU_ERR_ARG for a NULL pointer (inter may be NULL), whatever the state;
 * GPEMU_ERR_STATE without a prediction set-up on either context; then GPEMU_ERR_ARG for d < 2, a Matern model, contexts on
 * different devices or with different designs or regression orders, a non-finite bound or hi_l <= lo_l, j == k or an index
 * outside 0 .. d - 1, npts < 1. */
int gpemu_sens_pairs(gpemu_ctx *a, gpemu_ctx *b /* may be a */, const double *lo, const double *hi /* d each, host */,
                     double *cov_pair /* npairs */);
int gpemu_sens_pairs_dev(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi /* HOST */, double *out_dev /* npairs */);
int gpemu_sens_pairs_post(gpemu_ctx *ctx, const double *lo, const double *hi /* d each, host */, double *s_pair /* npairs */);
int gpemu_sens_pairs_post_dev(gpemu_ctx *ctx, const double *lo, const double *hi /* HOST */, double *out_dev /* npairs */);
int gpemu_sens_joint(gpemu_ctx *ctx, const double *lo, const double *hi, int j, int k, int npts,
                     const double *xj, const double *xk /* npts each, host */, double *e0, double *joint /* npts */,
                     double *inter /* npts, may be NULL */);

/* ---- the input measure of the sensitivity entries -----------------
 * A property of the context, one kind per coordinate, as gpemu_set_mode is a property: no entry's signature changes.  The
 * stored kinds decide how EVERY gpemu_sens_* entry (host and _dev) reads lo_l and hi_l:
 *   GPEMU_MEASURE_UNIFORM   x_l uniform on [lo_l, hi_l]   (the default; the only measure before there was a switch)
 *   GPEMU_MEASURE_GAUSS     x_l ~ N(lo_l, hi_l^2): lo_l is the MEAN, hi_l the STANDARD DEVIATION
 * The coordinates stay independent.  With mean mu, variance sg^2, lengths s (context a) and t (b), a = x_il, b = x_i'l,
 * D1 = 1 + s sg^2, D2 = 1 + (s + t) sg^2, a Gaussian coordinate's one-dimensional integrals are Gaussians themselves:
 *   I_l(i)     = D1^-1/2 exp(-(s / D1) (a - mu)^2 / 2)
 *   J^1 = I c,  J^2 = I (c^2 + v),  J^3 = I (c^3 + 3 c v),   c = (s sg^2 a + mu) / D1,  v = sg^2 / D1
 *   II_l(i,i') = D2^-1/2 exp(-[s t sg^2 (a - b)^2 + s (a - mu)^2 + t (b - mu)^2] / (2 D2))
 *   E x^n      : m_0 = 1, m_1 = mu, m_n = mu m_{n-1} + (n - 1) sg^2 m_{n-2}   (n <= 6)
 *   UU_l       = (1 + 2 s sg^2)^-1/2      (the prior double integral of gpemu_sens_post / _main_var / _pairs_post)
 * one exp and no erf; the three terms of II's exponent are all <= 0: no cancellation, no erfc case.  Everything is written in
 * sg^2, so very wide and very narrow measures stay finite.  Everything downstream of these five (the finishes, P, the band,
 * the leave-two-out products, the surfaces) does not know the measure.  A grid or surface value on a Gaussian coordinate is
 * any finite real.  The N x N sweeps have three instantiations per shape: all uniform (the code as it was, the same bits
 * as before the switch existed), all Gaussian (no erf code at all), and mixed (a branch per coordinate, uniform over a wave).
 * gpemu_sens_set_measure(ctx, kind): d values, or NULL for all uniform.  gpemu_set_model resets the kinds to all uniform (d
 * may change); gpemu_set_training, gpemu_predict_setup[_batch] and gpemu_sens_release keep them.  Errors: GPEMU_ERR_ARG for a
 * NULL ctx (for gpemu_sens_get_measure also a NULL kind) or a kind outside {0, 1} (nothing is stored then);
 * GPEMU_ERR_STATE before a model is set.
 * Argument checks of the sensitivity entries under a measure, still before anything is allocated or launched: a uniform
 * coordinate keeps its check (finite bounds, hi_l > lo_l); a Gaussian coordinate needs a finite mean and a finite standard
 * deviation > 0 -- hi_l <= lo_l is accepted there; in the two-context entries the kinds of a and b must agree, else
 * GPEMU_ERR_ARG.
 * Not built: correlated Gaussian inputs (a full covariance matrix), truncated Gaussians, Matern kernels. */
#define GPEMU_MEASURE_UNIFORM 0   /* x_l uniform on [lo_l, hi_l]            (the default) */
#define GPEMU_MEASURE_GAUSS   1   /* x_l ~ N(lo_l, hi_l^2): lo_l is the MEAN, hi_l the STANDARD DEVIATION */
int gpemu_sens_set_measure(gpemu_ctx *ctx, const int *kind /* d values, or NULL: all uniform */);
int gpemu_sens_get_measure(const gpemu_ctx *ctx, int *kind /* d */);

/* ---- implausibility and calibration likelihood against observations -----------------
 * Stands in for the reference's src/libRbind/implausOverDesign.R (computeImplaus, gridImplausComb) and adds the joint quantity
 * its interactive_mode leaves as a FIXME.  A multi-output emulator predicts y(x) = ybar + A m(x) with A = pca_evecs_r
 * sqrt(pca_evals_r) (nt x nr, row-major) and independent components of mean m_c(x) and variance v_c(x), D(x) = diag v(x).
 * Against observations z with covariance S (nt x nt, positive definite; or standard deviations sd: S = diag sd^2):
 *   chi2(x)   = (z - y(x))^T (S + A D A^T)^-1 (z - y(x))
 *   logpdf(x) = -1/2 (chi2 + log|S + A D A^T| + nt log 2 pi)       the joint log density of z: an MCMC likelihood
 *   I_t(x)    = |z_t - y_t| / sqrt(sum_c A_tc^2 v_c + S_tt + (rel_t y_t)^2)      the reference's per-output implausibility
 * (rel_t >= 0: a relative model error per output, the reference's errModel.sys; it enters the I_t alone).  Unlike sum_t I_t^2,
 * chi2 keeps the correlation between outputs that the back-projection creates.  No nt x nt work per point: once per
 * observation set (gpemu_calib_project, fp64 on the host, no device needed), with S = L_S L_S^T,
 *   G = A^T S^-1 A,   m_hat = G^-1 A^T S^-1 (z - ybar),   Sigma_z = G^-1,   c_perp = |L_S^-1 (z - ybar - A m_hat)|^2 >= 0
 * and per point, with delta = m(x) - m_hat and T(x) = Sigma_z + D(x),
 *   chi2 = c_perp + delta^T T^-1 delta,      log|S + A D A^T| = log|S| + log|G| + log|T|
 * one nr x nr Cholesky; D may be singular (a design point), nothing is a difference of large numbers.  c_perp is the misfit
 * no parameter value can remove (nt - nr degrees of freedom).
 * Limits: 1 <= nr <= nt, nr <= GPEMU_CALIB_MAX_R, nt <= GPEMU_CALIB_MAX_NT; beyond: GPEMU_ERR_ARG (not built).
 *
 * gpemu_calib_project: exactly one of S (nt x nt, both triangles; the lower one is read) and sd (nt) is given.  Outputs: mhat
 * (nr), sigz (nr x nr, symmetric bit for bit), consts = {c_perp, log|S|, log|G|}.  GPEMU_ERR_NOT_PD with the 1-based pivot in
 * *info when S or G is not positive definite to working precision (a pivot not above 64 eps times its diagonal element): for
 * G that means A has no full column rank; the outputs are then NaN.  GPEMU_ERR_ARG for a NULL pointer, both or neither of S
 * and sd, a size outside the limits, a non-finite input, sd <= 0.
 * gpemu_calib_setup runs the projection and keeps its tables resident on the context's device (ybar, A, z, S or sd, rel: HOST
 * arrays; rel may be NULL: none; a negative or non-finite rel is GPEMU_ERR_ARG).  The tables do not depend on the context's
 * model -- the context gives device, stream and error text --: gpemu_set_model leaves them alone, a second set-up replaces
 * them, gpemu_calib_release (waits for the stream) and gpemu_ctx_destroy free them.
 * gpemu_calib_eval: mean and var are component-major, row c at offset c * ld, ld >= M: what gpemu_predict_batch_dev of
 * component c writes.  A variance below 0 counts as 0 (kappa - |L^-1 k|^2 goes a few ulp negative at a design point).  stat
 * is 5 x M, statistic-major: row 0 chi2, row 1 logpdf, rows 2-4 the largest, second and third largest I_t (0 where nt < 3
 * leaves none); worst[q] = the output index of the largest I_t, the smallest index on a tie.  The sums over c run in index
 * order from 0.0, the order of the host layer's back-projection.  A NaN among a point's inputs makes that point's five
 * statistics NaN and its worst -1, no other point's.  A pivot <= 0 in T makes rows 0-1 of that point NaN; the call still
 * returns GPEMU_OK.  The _dev form only enqueues on the context's stream (one launch): the caller has ordered the producers
 * of mean and var.  GPEMU_ERR_STATE without a set-up; GPEMU_ERR_ARG for a NULL pointer, M < 1 or ld < M.
 * How it runs: one lane owns one query.  The lower triangle of T lives in registers, in instantiations for nr rounded up to 4,
 * 8, 12 and 16 (T padded with the identity, delta with 0: exact zeros in both sums), fully unrolled; the per-output rows of the
 * table (A, its squares, ybar, z, S_tt, rel) pass through LDS in chunks of 64 outputs, every lane of a wave reading the same
 * address.  Vector fp64, no matrix unit: 2 nt nr + nr^3 / 3 multiply-adds per point stand against the 2 N^2 per point and
 * component of the sweep it follows.
 * gpemu_calib_select: point q is kept iff stat[0][q] <= cut_chi2 and stat[1 + level][q] <= cut_I, level 1, 2 or 3 (the
 * reference's gridImplausComb is level 1).  INFINITY disables a cut; a NaN is never kept.  idx (M ints) receives the kept q in
 * ascending order, *count their number.  Per-workgroup counts, a scan, an ordered scatter: no atomics decide an output
 * position.  In the _dev form stat and idx are device pointers, count is a HOST int and the call waits for it.  Needs no
 * set-up.  GPEMU_ERR_ARG for a NULL pointer, M < 1, a level outside 1 .. 3 or a NaN cut.
 * gpemu_calib_gather_dev: the statistics of `count` listed points, point-major, out_dev[k * 5 + s] = stat[s][idx[k]], and (where
 * worst_dev and worst_out_dev are given) their worst outputs: what a caller downloads after a selection instead of all of
 * stat.  Only enqueues; an index outside 0 .. M-1 leaves its row unwritten.  GPEMU_ERR_ARG for a NULL pointer, M < 1 or
 * count < 0; count = 0 does nothing.
 * Two identical calls of any entry return the same bits; the host and _dev entries return the same bits.
 * Not built: nr > 16, nt > 1024; a mean-only pre-screen; the PCA truncation residual as an automatic addition to S (the caller
 * adds it to S).
 *
 * Gradients with respect to the query's coordinates.  With u = T^-1 delta and tau_c = (T^-1)_cc, for
 * coordinate j
 *   d chi2 / dx_j   =   2 sum_c u_c dm_c/dx_j  -      sum_c u_c^2 dv_c/dx_j
 *   d logpdf / dx_j =   - sum_c u_c dm_c/dx_j  +  1/2 sum_c (u_c^2 - tau_c) dv_c/dx_j
 * (c_perp, log|S| and log|G| are constants; d log|T| / dx_j = sum_c tau_c dv_c/dx_j).
 * gpemu_calib_grad: mean and var are exactly the inputs of gpemu_calib_eval; gmean and gvar hold component c's M x d row-major
 * block at offset c * ldg, ldg >= M * d: what gpemu_predict_mean_grad_dev and gpemu_predict_var_grad_dev of component c write.
 * gchi2 and glogpdf are M x d, point-major, g[q * d + j]; either may be NULL, not both.  A variance below 0 counts as 0 and
 * its dv_c then has weight 0: the derivative of the function gpemu_calib_eval evaluates.  A NaN among a point's means or
 * variances, or a pivot <= 0 in T, makes all 2 d values of that point NaN and no other point's; a non-finite gradient input
 * reaches its own (q, j) only.  Components beyond nr of the padded instantiation are never read.  The sums over c run in index
 * order from 0.0.  Two identical calls return the same bits, the host and the _dev form return the same bits, a point's bits
 * depend neither on M nor on its position in the call nor on which outputs are asked for; gpemu_calib_eval and every other
 * entry return the bits they returned before.  The _dev form only enqueues on the context's stream (one launch).
 * GPEMU_ERR_STATE without a set-up; GPEMU_ERR_ARG for a NULL input, both outputs NULL, M < 1, d < 1, ld < M or ldg < M * d.
 * How it runs: phase 1, one lane one query: the Cholesky of the evaluation in registers, u by the forward and the back solve,
 * tau_c as the squared norm of column c of L^-1 formed one column at a time; the weights go to LDS.  Phase 2, the workgroup's
 * lanes over the flat tile of its queries' outputs: every load of gmean, gvar and every store is unit-stride across the wave
 * for any d.  No atomics; 16 nr d bytes are read per point.
 * Not built: derivatives of the I_t (a max-type statistic); second derivatives; an optimiser on top (the sampler
 * below uses no gradient). */
#define GPEMU_CALIB_MAX_R  16
#define GPEMU_CALIB_MAX_NT 1024
int gpemu_calib_project(int nt, int nr, const double *ybar /* nt */, const double *A /* nt*nr */, const double *z /* nt */,
                        const double *S /* nt*nt or NULL */, const double *sd /* nt or NULL */, double *mhat /* nr */,
                        double *sigz /* nr*nr */, double *consts /* 3 */, int *info);
int gpemu_calib_setup(gpemu_ctx *ctx, int nt, int nr, const double *ybar, const double *A, const double *z, const double *S,
                      const double *sd, const double *rel /* nt or NULL */, int *info);
int gpemu_calib_release(gpemu_ctx *ctx);
int gpemu_calib_eval(gpemu_ctx *ctx, int M, const double *mean /* nr rows of ld, host */, const double *var, int ld,
                     double *stat /* 5*M */, int *worst /* M */);
int gpemu_calib_eval_dev(gpemu_ctx *ctx, int M, const double *mean_dev, const double *var_dev, int ld, double *stat_dev,
                         int *worst_dev);
int gpemu_calib_grad(gpemu_ctx *ctx, int M, int d, const double *mean /* nr rows of ld, host */, const double *var, int ld,
                     const double *gmean /* nr blocks of ldg, host */, const double *gvar, long ldg,
                     double *gchi2 /* M*d, may be NULL */, double *glogpdf /* M*d, may be NULL */);
int gpemu_calib_grad_dev(gpemu_ctx *ctx, int M, int d, const double *mean_dev, const double *var_dev, int ld,
                         const double *gmean_dev, const double *gvar_dev, long ldg, double *gchi2_dev, double *glogpdf_dev);
int gpemu_calib_select(gpemu_ctx *ctx, int M, const double *stat /* 5*M host */, double cut_chi2, int level, double cut_I,
                       int *idx /* M */, int *count);
int gpemu_calib_select_dev(gpemu_ctx *ctx, int M, const double *stat_dev, double cut_chi2, int level, double cut_I, int *idx_dev,
                           int *count /* HOST */);
int gpemu_calib_gather_dev(gpemu_ctx *ctx, int M, const double *stat_dev, const int *worst_dev /* may be NULL */, int count,
                           const int *idx_dev, double *out_dev /* count*5 */, int *worst_out_dev /* may be NULL */);

/* ---- posterior samples of the parameters: ensemble MCMC on the device -----------------
 * The affine-invariant ensemble sampler of Goodman & Weare 2010 (the stretch move) in the parallel half-ensemble form of
 * Foreman-Mackey et al. 2013, over log posterior = logpdf of gpemu_calib_eval + log prior.  No gradient, no proposal scale to
 * tune; a half-step evaluates W / 2 proposals in ONE gpemu_predict_batch_dev sweep per component plus ONE gpemu_calib_eval_dev
 * launch, and proposals, random numbers, the accept step and the trace stay on the device.
 *
 * Random numbers, specified to the bit: Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants
 * 0x9E3779B9 and 0xBB67AE85), key (seed & 0xffffffff, seed >> 32).  A uniform is made from two words,
 *   U(a, b) = (((uint64) a << 20 | b >> 12) + 0.5) 2^-52
 * strictly inside (0, 1), exact in fp64, the same bits on host and device.  Walker k at global step t: counter (k, t &
 * 0xffffffff, t >> 32, 0) gives words w0 .. w3, u1 = U(w0, w1), u2 = U(w2, w3); counter (k, t lo, t hi, 1) gives u3 = U(w0, w1).
 * A walker is active in exactly one half-step of a step: no counter repeats.  gpemu_philox4x32 and gpemu_sample_uniforms (u =
 * {u1, u2, u3}) are that generator on the host, the kernels' own body: they need no device.  GPEMU_ERR_ARG for a NULL pointer.
 *
 * State: x is W x d row-major, W even; lp is W values, log likelihood + log prior; half 0 is walkers 0 .. W/2 - 1, half 1 the rest.
 * gpemu_sample_set_prior(ctx, d, kind, lo, hi): a per-coordinate prior table resident on the context, in the convention of
 * gpemu_sens_set_measure (kind NULL: all uniform; for GPEMU_MEASURE_GAUSS lo is the mean and hi the standard deviation), with
 * its argument checks: GPEMU_ERR_ARG for a kind outside {0, 1}, lo >= hi on a uniform coordinate, a standard deviation <= 0, a
 * non-finite value, d outside 1 .. GPEMU_MAX_PARAMS, a NULL lo or hi.  Log prior of a point: a uniform coordinate gives
 * -log(hi - lo) inside [lo, hi], ends included, -inf outside (a NaN is outside); a Gaussian one -r^2 / 2 - log sd - log(2 pi) / 2;
 * summed over the coordinates in index order from 0.0.  The table does not depend on the model: gpemu_set_model leaves it, a
 * second call replaces it, gpemu_sample_release (waits for the stream; frees the run's buffers too) and gpemu_ctx_destroy free it.
 * gpemu_sample_propose_dev, active walker k of `half`, local index i: partner j = base of the other half + min(floor(u1 W/2),
 * W/2 - 1); z = ((a - 1) u2 + 1)^2 / a; y_i = x_j + z (x_k - x_j) into y_dev (W/2 x d row-major); aux_dev[i] = (d - 1) log z
 * (exactly 0 for d = 1); aux_dev[W/2 + i] = log prior of y_i.  One launch; every load of the walkers' own rows and every store
 * is unit-stride across a wave for any d (the lanes walk the flat tile of 64 walkers' coordinates); nothing outside y_dev and
 * aux_dev is written.  z and y are formed without contraction: +, * and / round once each, as a host would.
 * gpemu_sample_accept_dev: lp_y = loglik[i] + aux[W/2 + i]; the proposal is taken iff lp_y is finite and log u3 < aux[i] + lp_y
 * - lp_k (strict).  Taken: row k of x becomes row i of y bit for bit, lp_k becomes lp_y, naccept[k] grows by 1; not taken:
 * nothing of walker k changes; the other half is never touched.  One launch, no atomics: a walker has one owner.  loglik_dev is
 * row 1 of gpemu_calib_eval_dev's stat for M = W/2, but any pointer serves.
 * gpemu_sample_logpost_dev: lp[q] = loglik[q] + log prior of row q of x (M x d): how a run's start gets its lp.  One launch.
 * Errors of the three: GPEMU_ERR_ARG for a NULL pointer, odd W, W < 2 (logpost: M < 1), d outside 1 .. GPEMU_MAX_PARAMS, half
 * outside {0, 1}, a <= 1 or non-finite; GPEMU_ERR_STATE without a prior of that d.  All only enqueue on the context's stream.
 *
 * gpemu_calib_sample: comp[c] are the nr component contexts, each with a prediction set-up; obs holds the calibration set-up (its
 * nr equal to the argument) and the prior; obs may be one of the components; all on one device.  Start-up: lp of x0 by
 * gpemu_predict_batch_dev, gpemu_calib_eval_dev and gpemu_sample_logpost_dev in two half-batches of W/2; GPEMU_ERR_ARG if a start
 * has a non-finite lp.  Then for global step g = first_step + t, t = 0 .. nsteps - 1, half 0 then half 1: propose;
 * gpemu_predict_batch_dev of every component into component-major rows, ld = W/2; gpemu_calib_eval_dev; accept.  After step g,
 * if g >= burn and (g + 1) % thin == 0, x and lp are appended to a device-resident trace (trace_x: nrec x W x d, trace_lp: nrec x
 * W; either may be NULL, with both NULL nothing is staged); burn and thin count GLOBAL steps, so a run split into two calls
 * records the same steps.  *nrec_out = the records of this call.  The trace is staged in chunks of at most 64 MiB of records
 * (at least one record) and copied out chunk by chunk; gpemu_test_sample_chunk(ctx, records) sets another bound for tests (0: the
 * default).  naccept counts every step of the call.  x_end, lp_end: the ensemble after the last step.
 * The component streams and obs's stream are ordered with events (as gpemu_sens_cov orders two contexts): no host wait inside a
 * chunk of steps; the host waits where a chunk is copied out, once after the start-up evaluation and at the end.  Every buffer
 * of a run belongs to the sample state on obs, allocated once per call shape and reused; nothing is allocated inside the step loop.
 * Errors: GPEMU_ERR_ARG for a NULL required pointer, nr < 1, odd W, W/2 < d + 1 (each half must span the space), nsteps < 1, burn
 * < 0, thin < 1, a <= 1, contexts on different devices (not built) or with different d; GPEMU_ERR_STATE for a missing prediction
 * set-up, calibration set-up or prior (of the components' d), or a calibration nr different from the argument.
 * Guarantees: two identical calls return the same bits; a run of T steps equals, bit for bit, a run of T1 steps followed by one of
 * T - T1 steps with first_step = T1 from the first run's x_end (the traces concatenate, naccept adds up); the run equals, bit for
 * bit, the same sequence of the public entries issued one by one by a caller with a sync between them; every other entry
 * returns the bits it returned before.
 * Not built: gradient-based moves (MALA, HMC: the variance-gradient sweep costs about 20 prediction sweeps); other ensemble
 * moves; parallel tempering; components on several devices; convergence diagnostics beyond the host layer's integrated
 * autocorrelation time; starting from the non-implausible set; graph capture of a step. */
int gpemu_philox4x32(const unsigned ctr[4], const unsigned key[2], unsigned out[4]);
int gpemu_sample_uniforms(unsigned long long seed, unsigned walker, unsigned long long step, double u[3]);
int gpemu_sample_set_prior(gpemu_ctx *ctx, int d, const int *kind /* d values, or NULL: all uniform */, const double *lo, const double *hi);
int gpemu_sample_release(gpemu_ctx *ctx);
int gpemu_sample_propose_dev(gpemu_ctx *ctx, int W, int d, int half, unsigned long long step, unsigned long long seed, double a,
                             const double *x_dev /* W*d */, double *y_dev /* W/2*d */, double *aux_dev /* W */);
int gpemu_sample_accept_dev(gpemu_ctx *ctx, int W, int d, int half, unsigned long long step, unsigned long long seed,
                            const double *y_dev, const double *aux_dev, const double *loglik_dev /* W/2 */, double *x_dev,
                            double *lp_dev /* W */, int *naccept_dev /* W */);
int gpemu_sample_logpost_dev(gpemu_ctx *ctx, int M, int d, const double *x_dev /* M*d */, const double *loglik_dev /* M */,
                             double *lp_dev /* M */);
typedef struct gpemu_sample_args {
	int nwalkers, nsteps, burn, thin;
	unsigned long long seed, first_step;
	double a;
} gpemu_sample_args;
int gpemu_calib_sample(gpemu_ctx *const *comp, int nr, gpemu_ctx *obs, const gpemu_sample_args *args,
                       const double *x0 /* W*d host */, double *trace_x /* nrec*W*d or NULL */, double *trace_lp /* nrec*W or NULL */,
                       double *x_end /* W*d */, double *lp_end /* W */, int *naccept /* W */, int *nrec_out);
int gpemu_test_sample_chunk(gpemu_ctx *ctx, int records);

/* ---- low-level compatibility with the reference's host-matrix interface (what libRbind links against) ------
 * a14 chol_inverse_cov_matrix (libEmu/emulate-fns.c:275-299): the n x n matrix a (row stride lda, lower triangle
 * read) is replaced by its inverse (both triangles); *logdet = 2 sum log L_ii; *info as gpemu_loglik. */
int gpemu_chol_inverse(gpemu_ctx *ctx, int n, double *a_inout, int lda, double *logdet, int *info);
/* the C^-1-times-vector products of estimateBeta / getLogLikelyhood / makeEmulatedMean / makeEmulatedVariance
 * (libEmu/regression.c:120-176, estimator-fns.c:38-103, emulator.c:672-785) with C^-1 passed in host memory:
 * out[v*n + i] = sum_j a[i*lda + j] * v_rows[v*n + j] for nvec vectors stored as rows.  The matrix is uploaded when
 * its (pointer, size, 64-bit checksum over ALL its elements) differs from the copy the context holds: callers such as
 * the libRbind loops rewrite one cinverse buffer in place.  Cost per call with an unchanged matrix: one checksum pass
 * over its n*n doubles in host memory (0.1 s at n = 8192) -- gpemu_symm_pin(ctx, 1) is the caller's promise that the
 * buffer stays as it is until gpemu_symm_pin(ctx, 0) / gpemu_symm_invalidate, and removes that pass (the reference's
 * per-point loops over one cinverse, emulator.c:672-785, are such callers).  gpemu_symm_invalidate drops the cached
 * copy: the next call uploads without comparing. */
int gpemu_symm_apply(gpemu_ctx *ctx, int n, const double *a, int lda, int nvec, const double *v_rows, double *out_rows);
int gpemu_symm_invalidate(gpemu_ctx *ctx);
int gpemu_symm_pin(gpemu_ctx *ctx, int pinned);
/* a5 derivative_l_gauss (libEmu/emulator.c:173-209) written out: out[i*ldo + j] = exp(-0.5 e^{-2t} D^2 - 2t) D^2,
 * D = xcol[i] - xcol[j] (the ONE design coordinate the reference's formula looks at), t = theta_len */
int gpemu_derivative_gauss(gpemu_ctx *ctx, int n, const double *xcol, double theta_len, double *out, int ldo);
/* getGradientCn's trace(C^-1 dC/dtheta) (libEmu/maxmultimin.c:583-588): sum_ij a[i][j] b[j][i] of two host matrices,
 * one pass over both instead of the reference's N^3 dgemm */
int gpemu_trace_product(gpemu_ctx *ctx, int n, const double *a, int lda, const double *b, int ldb, double *trace);

/* ---- device memory helpers for callers that keep data resident ------ */
int gpemu_dev_alloc(gpemu_ctx *ctx, size_t bytes, void **dptr);
int gpemu_dev_free(gpemu_ctx *ctx, void *dptr);
int gpemu_dev_upload(gpemu_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int gpemu_dev_download(gpemu_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int gpemu_sync(gpemu_ctx *ctx);

/* ---- measurement: HIP-event timing of the kernels on ctx's stream ---
 * gpemu_prof_begin arms per-kernel-class event timing; every launch of that
 * class between begin and end is bracketed by hipEvents on the ctx stream.
 * gpemu_prof_end returns the number of launches and their summed duration. */
#define GPEMU_PROF_NONE    0
#define GPEMU_PROF_GEMM    1   /* f64 MFMA trailing-update / prediction GEMM */
#define GPEMU_PROF_FILL    2   /* covariance fill */
#define GPEMU_PROF_LEAF    3   /* diagonal-block factor + panel solve */
#define GPEMU_PROF_POTRF   4   /* whole factorisation (graph launch) */
#define GPEMU_PROF_GEMM_BIG 5  /* only the GEMM launches on the 128x128 8-wave kernel (the dominant kernel of a batch) */
#define GPEMU_PROF_GEMM_K512 6 /* only the GEMM launches with a contraction length >= 512 */
#define GPEMU_PROF_LOO     7   /* the two launches of gpemu_loo[_dev]: column sums over L^-1 (bytes = 8 N (N+1) / 2), finish */
#define GPEMU_PROF_MEAN    8   /* the two launches of the mean-only sweep: flops = M*N*(kernel + 2) with kernel = 3 d (the squared distance), bytes = 8*M*(d+1) */
#define GPEMU_PROF_MEAN_GRAD 9 /* the two launches of the mean-gradient sweep: flops = M*N*(3 d + 2 + 2 (d + 1)), bytes = 8*M*(2 d + 1) */
#define GPEMU_PROF_VAR_GRAD 10 /* the fused sweep of the variance-gradient entry and its finish: flops = M*N*(3 d + 1 + 2 (d + 1)), bytes = 8*M*(N + 2 d); its two products report under GPEMU_PROF_GEMM */
#define GPEMU_PROF_COV     11  /* the prior and mirror launches of gpemu_predict_cov[_dev]: bytes = 8*M*M (the lower triangle written once, mirrored once); its symmetric product reports under GPEMU_PROF_GEMM */
#define GPEMU_PROF_JOINT   12  /* the staging and clean launches of gpemu_predict_joint_factor[_dev] (bytes = 8*(64 M' + 2 M) and 4*M'*M', M' = M rounded up to 64) and the staging launch of every block of gpemu_predict_joint_draw[_dev] (bytes = 8*ndraw*(M' + 2 M)); the sweep, the products and the factorisation report under GPEMU_PROF_FILL / _COV / _GEMM / _LEAF / _POTRF */
#define GPEMU_PROF_LGO     13  /* the three launches per chunk of gpemu_lgo[_dev], nbc groups padded to bp: gather (bytes = 8 nbc bp Np: the rows of Z written; it reads at most the lower tiles of L^-1 besides), staging (bytes = 8 nbc bp (2 bp + 64): the lower tiles read and written, right-hand-side and identity rows written), finish (bytes = 8 nbc bp (bp / 2 + 4)); the product and the factorisation report under GPEMU_PROF_GEMM / _LEAF / _POTRF */
#define GPEMU_PROF_SENS    14  /* the three launches of gpemu_sens_cov[_dev] -- prep (flops = 88 N d: both contexts, two erf and two exp per point and coordinate counted as one flop each; bytes = 8 (10 N d + N d): the tables written, the design read), sweep (flops = N^2 (19 d + 2): per pair and coordinate one exp and two erf or erfc counted as one flop each among 16 others, then the 2 d + 1 sums; bytes = 8 T: the T = ceil(N / 64)^2 (2 d + 1) partial sums written), finish (flops = T, bytes = 8 T) -- and the two of gpemu_sens_main: prep, curves (flops = 6 N d ngrid, bytes = 16 d ngrid) */
#define GPEMU_PROF_SENS_POST 15 /* the four launches of gpemu_sens_post[_dev], L = n (n + 1) / 2 lower tiles with n = ceil(N / 64) -- prep (as GPEMU_PROF_SENS), pmat (flops = L (128 nreg^2 + 4096 (2 nreg + 1)): G for the tile's 64 rows, then a product of length nreg per pair; bytes = 8 * 8192 L: the corner's tile read, P's written), weighted sweep (flops = 4096 L (20 d + 3): the pair terms of GPEMU_PROF_SENS with one product more per coordinate and the rank-one sum; bytes = 8 (4096 L + T'), T' = L (2 d + 2): P read, the partial sums written), finish (flops = T' + (2 d + 2) nreg (2 nreg + 4 N), bytes = 8 (T' + (2 d + 2) 3 N nreg)) -- and of gpemu_sens_main_var: prep, then per block of mb rows tvec (flops = 6 mb N, bytes = 8 mb' Np, mb' = mb rounded up to 64) and band finish (flops = mb (2 Np + 2 nreg^2), bytes = 8 mb (Np + 64)); the corner and the band's product report under GPEMU_PROF_GEMM */
#define GPEMU_PROF_CALIB   16  /* the launch of gpemu_calib_eval[_dev] (flops = M (4 nt R + 8 nt + R^3 / 3 + 2 R^2), R = nr rounded up to 4: two multiply-adds per output and component, the finish of an output, the Cholesky and the solve in T; bytes = 8 M (2 nr + 5) + 4 M: mean and var read, stat and worst written) and the three of gpemu_calib_select[_dev], bracketed as ONE entry: count (16 M bytes: two rows of stat read), scan (8 ceil(M / 1024)), scatter (16 M + 4 kept, counted with kept = M), bytes = 36 M + 8 ceil(M / 1024), no flops */
#define GPEMU_PROF_DESIGN  17  /* the launches of gpemu_design_gain[_dev] that are its own: prep (as GPEMU_PROF_SENS), kmat when [K ; HK] is rebuilt (flops = 19 d N^2 / 2, bytes = 8 Np (Np + 64)), then per block of mb candidates their prep, kvec (flops = mb N (3 d + 2), bytes = 8 mb' Np), the transpose of a (bytes = 16 mb' Np), the cross sweep (flops = mb N (19 d + 4), bytes = 8 mb (2 N + ceil(N / 64))) and the finish (flops = mb (2 Np + 2 nreg^2 + 19 d), bytes = 8 mb (Np + 64)); the three products report under GPEMU_PROF_GEMM */
#define GPEMU_PROF_DESIGN_TARGET 18 /* the launches of gpemu_design_target_set / _gain[_dev] that are their own: per block of mb points the k fill (flops = mb N (3 d + 2), bytes = 8 mb' Np); per panel of ns targets the sweep (flops = mb ns (3 d + 2 nreg + 25), bytes = 8 mb (ns + ceil(ns / 64))) and the finish (flops = mb ceil(ns / 64), bytes = 8 mb (ceil(ns / 64) + 3)); the sum of target_var (flops = 2 S, bytes = 16 S); the products, the prediction's finish and Q r report under GPEMU_PROF_GEMM or not at all */
/* GPEMU_PROF_SENS*, under a measure (gpemu_sens_set_measure): in every sweep a GAUSSIAN coordinate's pair factor counts 12
 * flops (one exp among 11 others) where a uniform one counts 19 (one exp and two erf or erfc among 16): 19 d above becomes
 * 19 d_u + 12 d_g, and in the pair sweeps the 8 / 16 factors of a block are taken in the proportion d_u : d_g.  The prep and
 * finish counts are kept as they are (a Gaussian coordinate's tables cost one exp, not two erf and two exp: an upper bound). */
int gpemu_prof_begin(gpemu_ctx *ctx, int kernel_class);
int gpemu_prof_end(gpemu_ctx *ctx, int *nlaunches, double *total_ms, double *flops, double *bytes);

/* Diagnostics: with GPEMU_TRACE=1 in the environment at gpemu_ctx_create, every GEMM / leaf kernel of a
 * factorisation records (one workgroup in 16) its start and end on the device wall clock; this writes one line
 * per launch of the last factorisation:
 *   tag | start_ns end_ns sum_of_workgroup_ns workgroups sum_of_workgroup_shader_clocks stamp1 stamp2 stamp3
 * (stamps, in shader clocks since the workgroup started: GEMM prologue end / epilogue length / -; leaf factor:
 * block staged / first 16-column panel factored / first rank-16 update done)
 * Contexts of one GPU share the clock, so the files of concurrent contexts merge into one timeline
 * (tools/trace_timeline.py). */
int gpemu_trace_dump(gpemu_ctx *ctx, const char *path);

/* ---- low-level building blocks exported for parity tests ------------ */
/* C[m*n] = beta*C + alpha * A[m*K] * B[n*K]^T, host row-major buffers; beta is 0 or 1, and with beta = 1
 * alpha must be +1 or -1 (the accumulators start from C/alpha) */
int gpemu_test_gemm_nt(gpemu_ctx *ctx, int m, int n, int k, double alpha, int beta,
                       const double *a, const double *b, double *c);
/* ONE launch of the GEMM kernel in any of its modes, on operands inside one host buffer (the arena):
 *   C = beta*C + alpha * A[m x K] * B[n x K]^T over k in [k0, k1), C, A and B at element offsets offC/offA/offB.
 * tri: only tiles that meet the lower triangle are computed (elements above the diagonal inside them may or may not be
 * written).  kstart_mode: tiles skip k < floor16(first row - kstart_off), the caller promises A[i][k] = 0 for
 * k < i - kstart_off.  kend_mode: tiles skip k >= ceil16(last column + 1 - kend_off), the caller promises B[j][k] = 0 for
 * k > j - kend_off.  nbatch > 1: that many problems, bsC/bsA/bsB elements apart.  ksplit > 1: slice s of the k-range,
 * klen = ceil16(ceil((k1 - k0) / ksplit)) long, goes to C + s*bsC (beta = 0, one problem).  force_cfg: 2 = 64x64 tiles,
 * 8 = 128x128 tiles, 0 = the context's automatic choice.  fa: the workgroup of tile (0,0) leaves the updated 64x64 block
 * as its Cholesky factor (lower triangle; the part above the diagonal of that block is scratch), a failed pivot at
 * row r (1-based) of matrix b gives info_out[b] = fa_c0 + r, otherwise 0; needs tri, alpha = -1, beta = 1, 64x64 tiles.
 * The whole arena is uploaded, and downloaded after the launch.  GPEMU_ERR_ARG, before anything runs, if the launch
 * could address an element outside [0, arena_len), if k0 or k1 is no multiple of 16 or k1 <= k0, beta is not 0/1,
 * beta = 1 with alpha not +-1, ksplit > 1 with beta or nbatch > 1, force_cfg is not 0/2/8, or fa is set and the launch
 * would not take the factor-ahead tile.  info_out: max(nbatch, 1) words, may be NULL. */
typedef struct gpemu_gemm_launch_args {
	long offC, offA, offB;
	long ldc, lda, ldb;
	long bsC, bsA, bsB;
	double alpha;
	int m, n, k0, k1;
	int beta, tri;
	int kstart_mode, kstart_off, kend_mode, kend_off;
	int nbatch, ksplit, force_cfg;
	int fa, fa_c0;
} gpemu_gemm_launch_args;
int gpemu_test_gemm_launch(gpemu_ctx *ctx, double *arena, long arena_len, const gpemu_gemm_launch_args *args, int *info_out);
/* ONE trailing update of the factorisation, made exactly as production makes it, on tall matrices inside one host buffer
 * (the arena): matrix b at element offset off + b*stride is ld rows of ld columns (the matrix proper), rp right-hand-side
 * rows under them and, with inv, identity rows under those.  With P = rows c0+k .. of columns c0 .. c0+k-1 (the factored
 * panel), rows c0+k .. ld+rp-1 (inv: and c0+k more) of columns c0+k .. c0+k+ncols-1 become C - P P^T on and below the
 * diagonal of the matrix proper (tiles that meet it are computed whole or in part) and in every right-hand-side and identity
 * row.  rhs_live: how many of the rp right-hand-side rows can be non-zero (the others must be +0), 0 = unknown.  ride: the
 * GPEMU_RHS_RIDE switch for this call; the context's other switches apply as they are.  Where the update runs on 64x64 tiles
 * the factor-ahead rules of the context apply (info_out as gpemu_test_gemm_launch, max(nbatch, 1) words, may be NULL).
 * The whole arena is uploaded, and downloaded after the update.  GPEMU_ERR_ARG, before anything runs: a NULL pointer; k no
 * positive multiple of 16; c0 < 0, ncols < 1 or c0 + k + ncols > ld; rhs_live outside 0 .. rp; inv or ride not 0/1; nbatch
 * outside 0 .. GPEMU_MAX_BATCH; an odd off, ld, stride or c0; matrices of a batch that overlap; or a footprint -- rows
 * c0+k .. ld+rp(+c0+k)-1 of columns c0 .. c0+k+ncols-1 of every matrix -- that leaves [0, arena_len). */
typedef struct gpemu_update_launch_args {
	long off, ld, stride;
	int c0, k, ncols;
	int rp, inv;
	int rhs_live, nbatch, ride;
} gpemu_update_launch_args;
int gpemu_test_update_launch(gpemu_ctx *ctx, double *arena, long arena_len, const gpemu_update_launch_args *args, int *info_out);
/* ONE call of the Cholesky leaf launchers (the 64-column kernels of every factorisation) on a matrix inside one host
 * buffer (the arena), element offset off, row stride ld; nbatch > 1: that many matrices, bstride elements apart.
 *   GPEMU_LEAF_FACTOR        the 64x64 block at (c0, c0) leaves as its Cholesky factor: the lower triangle is L, the upper
 *                            16x16 blocks (0,1) (1,2) (2,3) (0,3) of it hold the inverses of L's diagonal 16x16 blocks
 *                            0, 1, 2, 3 (each a full 16x16 block, zero above its diagonal); blocks (0,2) (1,3) and the strict
 *                            upper triangles of the four diagonal 16x16 blocks are neither read nor written.  m_below = 0.
 *   GPEMU_LEAF_SOLVE         X L^T = B in place on rows c0+64 .. c0+64+m_below-1 of columns c0 .. c0+63, L the factored
 *                            block at (c0, c0).  staged: 1 / 0 = rows move as whole 512-byte pieces / as doubles, -1 = the
 *                            launch-size rule; pre: 1 = the diagonal inverses are read from the block's upper part, 0 = they
 *                            are computed from L (the upper part is not read).  c0b >= 0: one more workgroup solves the 64
 *                            rows under the factored block at (c0b, c0b), columns c0b .. c0b+63, the same way.
 *   GPEMU_LEAF_FACTOR_SOLVE  both, the plain leaf.
 *   GPEMU_LEAF_PAIR          the first block of a 128-column pair, m_below a multiple of 64: rows 64.. of the m_below rows
 *                            under the factored block (with its inverses) at (c0, c0) are solved as above; the FIRST 64 rows
 *                            of columns c0 .. c0+63 keep their bits (a later solve with c0b = c0 stores them); columns
 *                            c0+64 .. c0+127 of all m_below rows become C2 - X1 X0^T, X0 the solved first 64 rows.  fa: the
 *                            first 64 rows of those columns leave as the factor of the updated block, as GPEMU_LEAF_FACTOR
 *                            leaves it; without fa everything above that block's diagonal is unspecified.
 *   GPEMU_LEAF_PANEL_ROWS    the m_far rows from r_far on (m_far a multiple of 64, r_far >= c0 + 256) under the FINISHED
 *                            256-column group at c0 -- rows and columns c0 .. c0+255 hold L with the diagonal inverses of its
 *                            four 64x64 diagonal blocks -- leave, in columns c0 .. c0+255, with the bits the group's five
 *                            launches (pair, solve, K = 128 update, pair, solve) over those rows give them.  m_below = 0,
 *                            c0b = -1, fa = 0; the square is only read.
 * A pivot <= 0 or NaN at row r (1-based) of the block being factored gives info_out[b] = c0 + r (the pair's tile:
 * c0 + 64 + r) for matrix b, the first such row; otherwise 0.  Everything in a matrix whose pivot failed is unspecified.
 * Alignment contract: the staged solve and the pair move 16-byte pieces of rows, so off, ld, bstride, c0 and c0b must be
 * even (and the device allocation is 16-byte aligned).
 * The whole arena is uploaded, and downloaded after the launch; the device buffers are the call's own.
 * GPEMU_ERR_ARG, before anything runs: a NULL pointer; op, staged, pre, fa or c0b outside their values; nbatch outside
 * 0..GPEMU_MAX_BATCH; the pair with m_below < 64 or no multiple of 64; a solve with m_below < 1; the factor alone with
 * m_below != 0; an odd off, ld, bstride, c0 or c0b; c0b with an op that launches no solve; fa without the pair; columns
 * beyond ld; the panel rows with m_far < 64 or no multiple of 64, r_far < c0 + 256, m_below != 0, c0b or fa; r_far or m_far
 * != 0 with any other op; or any matrix whose footprint -- rows c0 .. c0+64+m_below-1 of columns c0 .. c0+63 (pair:
 * .. c0+127), rows c0b .. c0b+127 of columns c0b .. c0b+63, the panel rows: rows c0 .. c0+255 and r_far .. r_far+m_far-1 of
 * columns c0 .. c0+255 -- leaves [0, arena_len).  info_out: max(nbatch, 1) words. */
#define GPEMU_LEAF_FACTOR 0
#define GPEMU_LEAF_SOLVE 1
#define GPEMU_LEAF_FACTOR_SOLVE 2
#define GPEMU_LEAF_PAIR 3
#define GPEMU_LEAF_PANEL_ROWS 4
typedef struct gpemu_leaf_launch_args {
	long off, ld, bstride;
	int nbatch, c0, m_below;
	int op;
	int staged, pre, c0b, fa;
	int r_far, m_far;    /* GPEMU_LEAF_PANEL_ROWS only, otherwise 0 */
} gpemu_leaf_launch_args;
int gpemu_test_leaf_launch(gpemu_ctx *ctx, double *arena, long arena_len, const gpemu_leaf_launch_args *args, int *info_out);
/* The gradient's reduction kernels -- beta on the device, alpha, the tile sums of the literal or the exact form, their
 * second-stage sums: everything a value+gradient batch runs behind its C^-1 corners, through the routine production calls
 * -- ONCE on caller-chosen operands, for the model (design, covariance function) and the mode the context holds, nb
 * elements in lock-step.  Per element b:
 *   thetas  nthetas values, used as they come (amplitude e^theta0 for pow-exp and, GPEMU_MODE_MATERN_LOG, the Matern kernels)
 *   a       N x N, only the lower triangle is read: stands for C^-1
 *   z       N x (1 + nreg): stands for C^-1 [y|H]
 *   gram    (1 + nreg) x (1 + nreg), exact form only: gram[1+i][1+j] = (H^T C^-1 H)_ij, gram[1+i][0] = (H^T C^-1 y)_i
 * form: 0 = literal, 1 = exact.  gram_dist (exact form): 1 / 0 = tile distances from the matrix unit / from coordinate
 * differences, -1 = the context's GPEMU_GRAD_GRAM switch.  clamp (literal form): 1 / 0 = the kernel with / without the
 * lower bound on the exp argument, -1 = production's rule (without, when 1/2 e^{-2 theta_k} range_k^2 < 600 for every
 * direction and element).
 * Outputs: alpha_out nb x N; beta_out nb x nreg (exact form); part_out nb x ntiles x (2d + 2), tile t = tr (tr + 1) / 2
 * + tc of the 64 x 64 lower tiles; sums_out nb x (2d + 2).  Slots, literal: 2k = e^{-2 t_k} sum w a_ab D_k^2
 * exp(-1/2 e^{-2 t_k} D_k^2), 2k + 1 = the same with alpha_a alpha_b, 2d = sum a_aa, 2d + 1 = sum alpha_a^2 (diagonal
 * tiles); exact: k < nd = sum w (a_ab - alpha_a alpha_b) dC_ab/dtheta_k (nd = d for pow-exp, 1 for Matern), nd = the
 * nugget direction; w = 1 on the diagonal, 2 below it.  Slots the form does not define come back NaN, as everything the
 * kernels read beside their operands would make the outputs.  Uses device buffers of its own: the context's
 * factorisation, prediction state and result ring are not touched.
 * GPEMU_ERR_ARG, before anything runs: a NULL pointer, nb outside 1..GPEMU_MAX_BATCH, a switch outside its values, a
 * Matern model without GPEMU_MODE_EXACT_GRAD | GPEMU_MODE_MATERN_LOG or with form = 0, gram_dist = 1 on a design without a
 * centred copy, clamp = 0 where production's rule selects the clamped kernel. */
typedef struct gpemu_grad_sums_args {
	const double *thetas, *a, *z, *gram;
	double *alpha_out, *beta_out, *part_out, *sums_out;
	int nb, nthetas;
	int form, gram_dist, clamp;
} gpemu_grad_sums_args;
int gpemu_test_grad_sums(gpemu_ctx *ctx, const gpemu_grad_sums_args *args);
/* micro-benchmark of one GEMM shape on device-resident random operands: cfg 0 = the automatic tile choice, 2 = 64x64
 * tiles (4 waves), 8 = 128x128 tiles (8 waves); tri = lower-trapezoid update as in the factorisation; HIP-event timed. */
int gpemu_test_gemm_bench(gpemu_ctx *ctx, int m, int n, int k, int ld, int cfg, int tri, int beta, int reps,
                          double *ms_avg, double *flops);
/* in-place lower Cholesky of a host n*n matrix (both triangles read as lower);
 * returns L in the lower triangle, zeros above. */
int gpemu_test_potrf(gpemu_ctx *ctx, int n, double *a, int *info);
/* the matrix a lock-step batch is factored FROM: stages nb matrices as gpemu_loglik_batch does (one launch of the batch
 * staging kernel, lower tiles only) and copies the N x N block of matrix b to out[N*N] without factorising; tiles
 * strictly above the diagonal are not written by that path. */
int gpemu_test_staged_matrix(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas, int b, double *out);
/* ONE call of a covariance fill launcher -- the launchers every likelihood, gradient and prediction starts from, unchanged --
 * for the model (design, its centred copy, covariance function) and the mode the context holds, into the host buffer out.
 * Np = N rounded up to 64; every region has Np columns and row stride Np.
 *   GPEMU_FILL_STAGE  the staging launch of a lock-step batch, lower tiles with identity padding: nb matrices with nb theta
 *                     vectors (nthetas apart); per matrix (Np + Rp + guard) rows, one matrix after the other.  Rows [0, Np):
 *                     the 64 x 64 tiles (tr, tc <= tr) hold cov(x_i, x_j) for i, j < N, 1 on the diagonal beyond N and 0
 *                     elsewhere; tiles strictly above the diagonal are not written.  Rows [Np, Np + Rp): a copy of the
 *                     right-hand-side rows rrows (Rp x Np, row stride Np): rstride = 0 the same block for every matrix,
 *                     otherwise matrix b takes rrows + b * rstride (0 <= rstride <= 4 * Rp * Np); rrows must hold
 *                     (nb - 1) * rstride + Rp * Np doubles, all of which are read.  Rp = 0: the context's 64; other values up to 256 are
 *                     staged the same way (in 64-row blocks of which rows >= Rp are not written).  The guard rows are not
 *                     written.  form: -1 = production's rule (the Gram-form kernel if every theta is admitted to the Gram
 *                     form, else the batch kernel, each matrix in its own form), 0 = the batch kernel, every matrix from
 *                     coordinate differences, 1 = the Gram-form kernel, 2 = the batch kernel, each matrix in its own form.
 *   GPEMU_FILL_KVEC   k-vectors of the M query rows xq (M x d) with the 1e-10 clamp: an Mp x Np block (Mp = M rounded up to
 *                     64), rows >= M and columns >= N zero, then guard rows that are not written.  nb = 1.  form: 1 = the
 *                     Gram-form kernel, 0 = the difference form, -1 = the prediction sweep's rule.
 *   GPEMU_FILL_FULL   the full matrix as gpemu_cov_matrix fills it (difference form, both triangles, zero padding): Np x Np,
 *                     then guard rows that are not written.  nb = 1, form = 0.
 * A theta is admitted to the Gram form while norm2 = sum_k (w_k * half range_k)^2 <= 16 (w_k the coordinate scale of its
 * length scale).  Per matrix, form_out[b] = 1 / 0: its elements came from the Gram form / from differences, and
 * norm2_out[b] = that norm2 (NaN for a design without a centred copy).
 * The whole region (out_len >= nb * rows per matrix * Np doubles) is uploaded before the launch and downloaded after it,
 * so the caller's prefill shows what was written.  Uses device buffers of its own: the context's factorisation workspace,
 * prediction state and result ring are not touched.
 * GPEMU_ERR_ARG, before anything runs: a NULL pointer (rrows for the staging, xq for k-vectors, thetas, out, form_out,
 * norm2_out); op or form outside their values; nb outside 1..GPEMU_MAX_BATCH, or not 1 for k-vectors and the full matrix;
 * nthetas too small for the covariance function; form = 1 with a theta that is not admitted or a design without a centred
 * copy; M < 1; guard or Rp negative or out of range; rstride outside 0 .. 4 * Rp * Np; out_len shorter than the footprint. */
#define GPEMU_FILL_STAGE 0
#define GPEMU_FILL_KVEC 1
#define GPEMU_FILL_FULL 2
typedef struct gpemu_fill_launch_args {
	const double *thetas, *rrows, *xq;
	double *out, *norm2_out;
	int *form_out;
	long out_len, rstride;
	int op, form, nb, nthetas;
	int M, Rp, guard;
} gpemu_fill_launch_args;
int gpemu_test_fill_launch(gpemu_ctx *ctx, const gpemu_fill_launch_args *args);
/* ONE call of a launcher that reads the device-resident factor of gpemu_predict_setup -- the launchers the one-query and
 * few-query prediction products, gpemu_loo and gpemu_lgo call, unchanged -- on operands of the caller's.  What these kernels
 * share: above its diagonal L^-1 holds exact zeros only inside the diagonal 16 x 16 blocks and nothing specified further out
 * (U = R^-T of leave-group-out likewise left of its diagonal), so none of that may reach an output.  LinvAug (lin, row
 * stride ld): rows [0, Np) = L^-1, row Np = gamma, rows Np+1 .. Np+nreg = W^T; betaq = beta (nreg) then Q (nreg x nreg).
 *   GPEMU_RES_SKINNY, GPEMU_RES_GEMV   Vp[s][q][n] = sum over k in slice s = [s klen, min((s+1) klen, K)), k < ke(n), of
 *                         Kq[q][k] L[n][k], ke(n) = (n & ~15) + 16 for n < ntri and K otherwise.  kq: 16 rows of stride ldk (the
 *                         one-query kernel reads row 0), lin: ntot rows of stride ld, vp: nslice x vrows x ldv.  The skinny
 *                         kernel writes rows 0 .. 15, the one-query kernel row 0, columns [0, ntot) of every slice.
 *   GPEMU_RES_LOO_COLSQ   part[c][j] = sum of (L^-1)_rj^2 over rows r of the 64-row chunk c with j <= r < N, for every column
 *                         j < Np of every launched (512-column strip, chunk) pair: chunk >= 8 * strip.  part: ceil(N/64) x Np.
 *   GPEMU_RES_LOO_FINISH  P_ii = sum_c part[c][i] - w_i^T Q w_i over the launched chunks, var_i = 1 / P_ii, mean_i = y_i -
 *                         gamma_i / P_ii for i < N.
 *   GPEMU_RES_LGO_GATHER  z (nbc x bp x Np): row colrow[i] - g0 bp, where inside the chunk, = column i of L^-1 from row i to
 *                         row N-1, zero elsewhere; the pad rows of every group zero.  Every element is written.
 *   GPEMU_RES_LGO_STAGE   the staging of nbc tall matrices t ((2 bp + 64) x bp each, tstride apart) whose lower 64 x 64 tiles
 *                         hold (C^-1)_BB: minus w_r^T Q w_c between members, identity at the pad, row bp = gamma at the
 *                         members, rows bp+1 .. bp+63 zero, then the identity rows.  Tiles above the diagonal are not touched.
 *   GPEMU_RES_LGO_FINISH  from factored tall matrices (row bp = the solved row w, rows bp+64 .. = U), info (nbc words as the
 *                         factorisation leaves them) and res ({|w|^2, 2 sum log R_ii} per group): var, mean, werr at the
 *                         members' design indices, stat (maha, logdet, logpdf: 3 x ngroups) and info_out (ngroups) at
 *                         g0 .. g0+nbc-1.  werr and stat may be NULL.
 *   GPEMU_RES_LGO_TAIL    everything gpemu_lgo runs per chunk behind the staging launch, on staged matrices t of the
 *                         caller's: the lock-step factorisation with inverse rows, |w|^2 and the log-determinant, the
 *                         finishing pass.  Outputs as GPEMU_RES_LGO_FINISH; returns what gpemu_lgo returns: GPEMU_ERR_NOT_PD
 *                         if info_out of a group of the chunk is not 0 (that group's outputs are NaN, the others valid).
 * Tables as gpemu_lgo builds them: colrow (N), members (nmembers), moff and bsize (ngroups).  Lengths the shape fixes: betaq
 * nreg + nreg^2, y N, res 2 nbc, info nbc, stat 3 ngroups, info_out ngroups; mean, var and werr hold out_len >= N each
 * (elements from N on are not written).
 * Every region the op takes is uploaded whole and downloaded whole after the launch, so the caller's prefill shows what was
 * written.  The device buffers are the call's own; no model is needed; the context's prediction state, factorisation
 * workspace and result ring are not touched.
 * GPEMU_ERR_ARG, before anything runs: a NULL pointer among the op's regions and tables; op outside its values; K or klen no
 * multiple of 16, ntot no multiple of 64, ntri no multiple of 16 or beyond ntot or K, nslice * klen < K, vrows < 16, ldv <
 * ntot; ld or ldk below K or no multiple of 4 (products), ld odd or below Np (the other ops that take lin); N outside
 * 1 .. Np or Np no multiple of 64 (the same ops; N < 1 for the others); nreg outside 1 .. 63 (the ops that take betaq); bp no multiple of 64, nbc outside 1 .. GPEMU_MAX_BATCH, g0 + nbc > ngroups; an odd tstride
 * or one below (2 bp + 64) bp; a group size outside 1 .. bp, members outside 0 .. N-1 or beyond nmembers, a colrow entry
 * outside -1 .. ngroups bp - 1; or a footprint beyond the given length of a region. */
#define GPEMU_RES_SKINNY 0
#define GPEMU_RES_GEMV 1
#define GPEMU_RES_LOO_COLSQ 2
#define GPEMU_RES_LOO_FINISH 3
#define GPEMU_RES_LGO_GATHER 4
#define GPEMU_RES_LGO_STAGE 5
#define GPEMU_RES_LGO_FINISH 6
#define GPEMU_RES_LGO_TAIL 7
typedef struct gpemu_resident_launch_args {
	double *lin, *kq, *vp, *part, *betaq, *y, *z, *t, *res, *mean, *var, *werr, *stat;
	const int *colrow, *members, *moff, *bsize, *info;
	int *info_out;
	long lin_len, ld, kq_len, ldk, vp_len, ldv, part_len, z_len, t_len, tstride, out_len;
	int op, K, ntri, ntot, nslice, klen, vrows;
	int N, Np, nreg, g0, nbc, bp, ngroups, nmembers;
} gpemu_resident_launch_args;
int gpemu_test_resident_launch(gpemu_ctx *ctx, const gpemu_resident_launch_args *args);
/* beta (nreg) and gamma = C^-1 (y - H beta) (N), bit for bit as the prediction state holds them in HBM.  For tests whose bar is
 * a few ulp (the closed-form sensitivity entries): their reference must start from these two vectors, since another
 * factorisation's gamma differs from the device's by far more than that.  GPEMU_ERR_STATE without a prediction set-up. */
int gpemu_test_pred_state(gpemu_ctx *ctx, double *beta, double *gamma);
/* the same for gpemu_sens_post: P = C^-1 - W Q W^T (N*N, both triangles), G = W Q (N*nreg) and Q (nreg*nreg), bit for bit what
 * the last call's weighted sweep and finish multiplied by.  GPEMU_ERR_STATE before the first gpemu_sens_post of a model. */
int gpemu_test_sens_post_state(gpemu_ctx *ctx, double *P /* N*N, both triangles */, double *G /* N*nreg */, double *Q /* nreg*nreg */);
/* the same for gpemu_design_gain: the rows of a = L^-T u + W Q r and of b = Q r of the last block of the last call, bit for bit
 * what its third product, sweep and finish multiplied by; npoints: that block's candidates (a call of up to 16 384 has one
 * block).  GPEMU_ERR_STATE when no block of this size was the last. */
int gpemu_test_design_state(gpemu_ctx *ctx, int npoints, double *a_out /* npoints*N */, double *b_out /* npoints*nreg */);
/* the same for gpemu_design_batch: lambda and mu (npoints x nbatch each) and E (nbatch x nbatch) of this context's part in the
 * last call, bit for bit; GPEMU_ERR_STATE where the last call had other sizes */
int gpemu_test_design_batch_state(gpemu_ctx *ctx, int npoints, int nbatch, double *lam_out, double *mu_out, double *e_out);
/* the same for gpemu_design_target_*: the rows of u (N each), r and Q r (nreg each), bit for bit what the panel product and
 * the sweep read.  which = 0: the resident store of the npoints targets; which = 1: the last block of candidates of the last
 * gain call (its u and Q r rows still lie in the prediction batch buffer: call it directly behind that gain call).
 * GPEMU_ERR_STATE where no store or block of this size is there. */
int gpemu_test_design_target_state(gpemu_ctx *ctx, int which, int npoints, double *u_out /* npoints*N */, double *r_out /* npoints*nreg */,
                                   double *qr_out /* npoints*nreg */);
/* the workgroup -> tile table of a GEMM launch with tiles_m x tiles_n tiles (tri = 1: lower triangle) and super-blocks
 * of sb x sb tiles: entry q * 8 + x is the q-th tile of XCD x, (tm << 16) | tn, or -1 (unused tail slot).  Host logic
 * only (no device).  Returns the table length, or -GPEMU_ERR_ARG; writes min(length, cap) entries to out. */
int gpemu_test_tile_table(int tiles_m, int tiles_n, int tri, int sb, int *out, int cap);
/* the table of the square product with row-start skipping (C^-1 = U U^T; tile (r, c <= r), tile row r contracting from
 * k = max(k0, floor16(r * bm - kstart_off)) to k1): whole tile rows per XCD, rows dealt longest-work-first to the least
 * loaded XCD, each XCD's rows by decreasing k-range.  Same entry format and return value as above. */
int gpemu_test_row_table(int tiles_m, int bm, int kstart_off, int k0, int k1, int *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* GPEMU_H */
