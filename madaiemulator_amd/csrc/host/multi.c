/*
 * multi.c -- multi-output models: PCA of the N x t training matrix, nr independent scalar GPs,
 * the MODEL_SNAPSHOT_FILE, and back-projection of predictions
 * (multi_modelstruct.c:38-507, multivar_support.c:20-157 of the reference).
 *
 * gsl_eigen_symmv is replaced by a cyclic Jacobi eigen-solver (nt is the number of outputs, tens
 * at most); eigenvector signs are whatever the solver returns, as with GSL -- only back-projected
 * outputs are comparable between implementations.
 */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <pthread.h>
#include "libemu.h"
#include "gpemu.h"

double vector_elt_sum(gsl_vector *vec, int nstop)
{
	assert(nstop >= 0);
	assert((unsigned)nstop <= vec->size);
	double sum = 0.0;
	for (int i = 0; i < nstop; i++) sum += gsl_vector_get(vec, i);
	return sum;
}

/* symmetric eigen-decomposition A = V diag(w) V^T by cyclic Jacobi rotations; A is n x n row-major and destroyed */
static void jacobi_eigen(double *A, int n, double *w, double *V)
{
	for (int i = 0; i < n; i++)
		for (int j = 0; j < n; j++) V[i * n + j] = (i == j) ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 100; sweep++) {
		double off = 0.0;
		for (int i = 0; i < n; i++)
			for (int j = i + 1; j < n; j++) off += A[i * n + j] * A[i * n + j];
		if (off < 1e-300) break;
		for (int p = 0; p < n - 1; p++)
			for (int q = p + 1; q < n; q++) {
				const double apq = A[p * n + q];
				if (apq == 0.0) continue;
				const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
				for (int k = 0; k < n; k++) {
					const double akp = A[k * n + p], akq = A[k * n + q];
					A[k * n + p] = c * akp - s * akq;
					A[k * n + q] = s * akp + c * akq;
				}
				for (int k = 0; k < n; k++) {
					const double apk = A[p * n + k], aqk = A[q * n + k];
					A[p * n + k] = c * apk - s * aqk;
					A[q * n + k] = s * apk + c * aqk;
				}
				for (int k = 0; k < n; k++) {
					const double vkp = V[k * n + p], vkq = V[k * n + q];
					V[k * n + p] = c * vkp - s * vkq;
					V[k * n + q] = s * vkp + c * vkq;
				}
			}
	}
	for (int i = 0; i < n; i++) w[i] = A[i * n + i];
}

/* multi_modelstruct.c:172-338 */
void gen_pca_decomp(multi_modelstruct *m, double vfrac)
{
	const int nt = m->nt, N = m->nmodel_points;
	double *ysub = (double *)malloc(sizeof(double) * (size_t)N * nt);
	double *cov = (double *)calloc((size_t)nt * nt, sizeof(double));
	double *w = (double *)malloc(sizeof(double) * (size_t)nt), *V = (double *)malloc(sizeof(double) * (size_t)nt * nt);
	for (int i = 0; i < nt; i++) {
		printf("# y(%d) mean: %lf\n", i, gsl_vector_get(m->training_mean, i));
		for (int j = 0; j < N; j++) ysub[j * nt + i] = gsl_matrix_get(m->training_matrix, j, i) - gsl_vector_get(m->training_mean, i);
	}
	for (int a = 0; a < nt; a++)
		for (int b = 0; b < nt; b++) {
			double s = 0.0;
			for (int j = 0; j < N; j++) s += ysub[j * nt + a] * ysub[j * nt + b];
			cov[a * nt + b] = s * (1.0 / (double)N);
		}
	jacobi_eigen(cov, nt, w, V);
	/* descending eigenvalues, eigenvectors in columns (gsl_eigen_symmv_sort ... GSL_EIGEN_SORT_VAL_DESC) */
	int *ord = (int *)malloc(sizeof(int) * (size_t)nt);
	for (int i = 0; i < nt; i++) ord[i] = i;
	for (int i = 0; i < nt; i++)
		for (int j = i + 1; j < nt; j++)
			if (w[ord[j]] > w[ord[i]]) { int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
	gsl_vector *evals = gsl_vector_alloc(nt);
	for (int i = 0; i < nt; i++) gsl_vector_set(evals, i, w[ord[i]]);
	const double total_variance = vector_elt_sum(evals, nt);
	/* the reference's loop (:267-272): frac is the share of the FIRST i values, tested before i is advanced,
	 * so one component more than needed is kept, capped at nt-1 */
	int i = 0;
	double frac = 0.0;
	while (frac < vfrac && (i + 1) < nt) {
		frac = (1.0 / total_variance) * vector_elt_sum(evals, i);
		i++;
	}
	m->nr = i;
	if (nt == 1) m->nr = 1;
	m->pca_evals_r = gsl_vector_alloc(m->nr);
	m->pca_evecs_r = gsl_matrix_alloc(nt, m->nr);
	fprintf(stderr, "# nr: %d frac: %lf\n", m->nr, frac);
	for (int r = 0; r < m->nr; r++) {
		gsl_vector_set(m->pca_evals_r, r, gsl_vector_get(evals, r));
		for (int t = 0; t < nt; t++) gsl_matrix_set(m->pca_evecs_r, t, r, V[t * nt + ord[r]]);
	}
	/* Z = Ysub U_r diag(lambda_r^-1/2) */
	m->pca_zmatrix = gsl_matrix_alloc(N, m->nr);
	for (int j = 0; j < N; j++)
		for (int r = 0; r < m->nr; r++) {
			double s = 0.0;
			for (int t = 0; t < nt; t++) s += ysub[j * nt + t] * gsl_matrix_get(m->pca_evecs_r, t, r);
			gsl_matrix_set(m->pca_zmatrix, j, r, s * (1.0 / sqrt(gsl_vector_get(m->pca_evals_r, r))));
		}
	gsl_vector_free(evals);
	free(ord); free(ysub); free(cov); free(w); free(V);
}

/* multi_modelstruct.c:121-146 */
void gen_pca_model_array(multi_modelstruct *m)
{
	m->pca_model_array = (modelstruct **)malloc(sizeof(modelstruct *) * (size_t)m->nr);
	for (int i = 0; i < m->nr; i++) {
		gsl_vector *z = gsl_vector_alloc(m->nmodel_points);
		for (int j = 0; j < m->nmodel_points; j++) gsl_vector_set(z, j, gsl_matrix_get(m->pca_zmatrix, j, i));
		m->pca_model_array[i] = alloc_modelstruct_2(m->xmodel, z, m->cov_fn_index, m->regression_order);
	}
}

/* multi_modelstruct.c:38-110 */
multi_modelstruct *alloc_multimodelstruct(gsl_matrix *xmodel_in, gsl_matrix *training_matrix_in, int cov_fn_index,
                                          int regression_order, double varfrac)
{
	assert(training_matrix_in->size1 == xmodel_in->size1);
	assert(training_matrix_in->size1 > 0);
	assert(training_matrix_in->size2 > 0);
	assert(xmodel_in->size2 > 0);
	if (regression_order < 0 || regression_order > 3) regression_order = 0;
	if (varfrac < 0 || varfrac > 1) varfrac = 0.95;
	if (cov_fn_index != MATERN32 && cov_fn_index != MATERN52) cov_fn_index = POWEREXPCOVFN;
	multi_modelstruct *m = (multi_modelstruct *)malloc(sizeof(multi_modelstruct));
	m->nt = (int)training_matrix_in->size2;
	m->nr = 0;
	m->nmodel_points = (int)xmodel_in->size1;
	m->nparams = (int)xmodel_in->size2;
	m->xmodel = xmodel_in;
	m->training_matrix = training_matrix_in;
	m->training_mean = gsl_vector_alloc(m->nt);
	m->regression_order = regression_order;
	m->cov_fn_index = cov_fn_index;
	for (int i = 0; i < m->nt; i++) {
		gsl_vector_view col = gsl_matrix_column(m->training_matrix, i);
		gsl_vector_set(m->training_mean, i, vector_elt_sum(&col.vector, m->nmodel_points) / (double)m->nmodel_points);
	}
	gen_pca_decomp(m, varfrac);
	gen_pca_model_array(m);
	return m;
}

/* multi_modelstruct.c:346-401 */
void dump_multi_modelstruct(FILE *fptr, multi_modelstruct *m)
{
	assert(fptr);
	fprintf(fptr, "%d\n", m->nt);
	fprintf(fptr, "%d\n", m->nr);
	fprintf(fptr, "%d\n", m->nparams);
	fprintf(fptr, "%d\n", m->nmodel_points);
	fprintf(fptr, "%d\n", m->cov_fn_index);
	fprintf(fptr, "%d\n", m->regression_order);
	for (int i = 0; i < m->nmodel_points; i++) {
		for (int j = 0; j < m->nparams; j++) fprintf(fptr, "%.17lf ", gsl_matrix_get(m->xmodel, i, j));
		fprintf(fptr, "\n");
	}
	for (int i = 0; i < m->nmodel_points; i++) {
		for (int j = 0; j < m->nt; j++) fprintf(fptr, "%.17lf ", gsl_matrix_get(m->training_matrix, i, j));
		fprintf(fptr, "\n");
	}
	for (int i = 0; i < m->nr; i++) fprintf(fptr, "%.17lf ", gsl_vector_get(m->pca_evals_r, i));
	fprintf(fptr, "\n");
	for (int i = 0; i < m->nt; i++) {
		for (int j = 0; j < m->nr; j++) fprintf(fptr, "%.17lf ", gsl_matrix_get(m->pca_evecs_r, i, j));
		fprintf(fptr, "\n");
	}
	for (int i = 0; i < m->nmodel_points; i++) {
		for (int j = 0; j < m->nr; j++) fprintf(fptr, "%.17lf ", gsl_matrix_get(m->pca_zmatrix, i, j));
		fprintf(fptr, "\n");
	}
	for (int i = 0; i < m->nr; i++) dump_modelstruct_2(fptr, m->pca_model_array[i]);
	/* Not in the reference's grammar, and invisible to its loader (which stops reading after the last modelstruct,
	 * multi_modelstruct.c:417-472): a Matern model trained with amplitude and nugget on the LOG scale says so.  Queried
	 * in the raw form its thetas would silently mean amp = theta0 instead of e^theta0.  Literal-mode snapshots (and every
	 * pow-exp one) carry no such line: they stay byte for byte what the reference writes. */
	if (m->cov_fn_index != POWEREXPCOVFN && (gpemu_host_modes() & 2 /* GPEMU_MODE_MATERN_LOG */))
		fprintf(fptr, "#gpemu matern_log_scale 1\n");
}

static int rd_int(FILE *f) { int v = 0; if (fscanf(f, "%d%*c", &v) != 1) { fprintf(stderr, "snapshot: read error\n"); gpemu_host_exit(EXIT_FAILURE); } return v; }
static double rd_dbl(FILE *f) { double v = 0; if (fscanf(f, "%lf%*c", &v) != 1) { fprintf(stderr, "snapshot: read error\n"); gpemu_host_exit(EXIT_FAILURE); } return v; }

/* multi_modelstruct.c:406-472 */
multi_modelstruct *load_multi_modelstruct(FILE *fptr)
{
	multi_modelstruct *m = (multi_modelstruct *)malloc(sizeof(multi_modelstruct));
	m->nt = rd_int(fptr);
	m->nr = rd_int(fptr);
	m->nparams = rd_int(fptr);
	m->nmodel_points = rd_int(fptr);
	m->cov_fn_index = rd_int(fptr);
	m->regression_order = rd_int(fptr);
	const int N = m->nmodel_points, nt = m->nt, nr = m->nr, d = m->nparams;
	m->xmodel = gsl_matrix_alloc(N, d);
	m->training_matrix = gsl_matrix_alloc(N, nt);
	m->training_mean = gsl_vector_alloc(nt);
	m->pca_model_array = (modelstruct **)malloc(sizeof(modelstruct *) * (size_t)nr);
	m->pca_evals_r = gsl_vector_alloc(nr);
	m->pca_evecs_r = gsl_matrix_alloc(nt, nr);
	m->pca_zmatrix = gsl_matrix_alloc(N, nr);
	for (int i = 0; i < N; i++) for (int j = 0; j < d; j++) gsl_matrix_set(m->xmodel, i, j, rd_dbl(fptr));
	for (int i = 0; i < N; i++) for (int j = 0; j < nt; j++) gsl_matrix_set(m->training_matrix, i, j, rd_dbl(fptr));
	for (int i = 0; i < nr; i++) gsl_vector_set(m->pca_evals_r, i, rd_dbl(fptr));
	for (int i = 0; i < nt; i++) for (int j = 0; j < nr; j++) gsl_matrix_set(m->pca_evecs_r, i, j, rd_dbl(fptr));
	for (int i = 0; i < N; i++) for (int j = 0; j < nr; j++) gsl_matrix_set(m->pca_zmatrix, i, j, rd_dbl(fptr));
	for (int i = 0; i < nr; i++) m->pca_model_array[i] = load_modelstruct_2(fptr);
	{
		/* the trailer dump_multi_modelstruct writes for log-scale Matern models: switch the layer to that mode */
		char line[128];
		int recorded = 0;
		while (fgets(line, sizeof line, fptr))
			if (!strncmp(line, "#gpemu matern_log_scale 1", 25)) recorded = 1;
		if (m->cov_fn_index != POWEREXPCOVFN) {
			const int have = (gpemu_host_modes() & 2) != 0;
			if (recorded && !have) {
				fprintf(stderr, "# snapshot: Matern thetas are on the log scale (trained with --matern_fixed): using that mode\n");
				gpemu_host_set_modes(gpemu_host_modes() | 2);
			} else if (!recorded && have) {
				fprintf(stderr, "# snapshot: no log-scale record in this Matern snapshot, but GPEMU_MATERN_FIXED is set: thetas are taken on the log scale\n");
			}
		}
	}
	for (int i = 0; i < nt; i++) {
		gsl_vector_view col = gsl_matrix_column(m->training_matrix, i);
		gsl_vector_set(m->training_mean, i, vector_elt_sum(&col.vector, N) / (double)N);
	}
	return m;
}

void free_multimodelstruct(multi_modelstruct *m)
{
	gsl_vector_free(m->training_mean);
	for (int i = 0; i < m->nr; i++) {
		gsl_vector_free(m->pca_model_array[i]->training_vector);
		gsl_matrix_free(m->pca_model_array[i]->xmodel);
		free_modelstruct_2(m->pca_model_array[i]);
	}
	free(m->pca_model_array);
	gsl_matrix_free(m->xmodel);
	gsl_matrix_free(m->training_matrix);
	gsl_vector_free(m->pca_evals_r);
	gsl_matrix_free(m->pca_evecs_r);
	gsl_matrix_free(m->pca_zmatrix);
	free(m);
}

/* multivar_support.c:20-28: the nr scalar GPs are independent; the reference trains them one after the other.  Here a
 * list of components is trained by a pool of host threads: component list[p] belongs to device slot p mod S
 * (S = gpemu_host_device_slots(), or the one device the caller is pinned to), and on every slot up to C components are
 * trained SIDE BY SIDE (GPEMU_COMPONENTS_PER_SLOT; default: as many of the slot's components as fit the device's free
 * memory with two lock-step groups each, at most 8) -- a search leaves the device idle between the rounds of its lock-step
 * groups (the BFGS arithmetic of its host threads, the latency-bound panel chains of its small batches), which the other
 * components' rounds fill.  Each thread runs the whole restart search of one component after the other on its slot's
 * device; no exchange between the threads -- the results meet in the modelstructs.  A component's search depends on the
 * seed, its data and the lock-step group size alone, not on which slot or thread ran it or what ran beside it, so the thetas
 * (and the snapshot) are the ones the serial loop gives. */
struct component_pool {
	multi_modelstruct *m;
	const int *list;             /* component indices of this slot, in order */
	int n, next;
	pthread_mutex_t mu;
	int device, share;
};

static void *component_main(void *arg)
{
	struct component_pool *P = (struct component_pool *)arg;
	gpemu_host_thread_device(P->device);
	gpemu_host_thread_share(P->share);
	for (;;) {
		pthread_mutex_lock(&P->mu);
		const int p = P->next < P->n ? P->next++ : -1;
		pthread_mutex_unlock(&P->mu);
		if (p < 0) break;
		modelstruct *c = P->m->pca_model_array[P->list[p]];
		estimate_thetas_threaded(c, c->options);
	}
	return NULL;
}

static void train_components(multi_modelstruct *m, const int *list, int nlist)
{
	if (nlist < 1) return;
	const int pinned = gpemu_host_thread_device_get();
	int nslots = pinned >= 0 ? 1 : gpemu_host_device_slots();
	if (nslots > nlist) nslots = nlist;
	int want = 0;                                                /* components side by side on one slot: 0 = by memory */
	const char *e = getenv("GPEMU_COMPONENTS_PER_SLOT");
	if (e && atoi(e) > 0) want = atoi(e);
	struct component_pool *pools = (struct component_pool *)calloc((size_t)nslots, sizeof *pools);
	int *order = (int *)malloc(sizeof(int) * (size_t)nlist), *nthreads = (int *)calloc((size_t)nslots, sizeof(int));
	int filled = 0, total_threads = 0;
	for (int s = 0; s < nslots; s++) {
		struct component_pool *P = &pools[s];
		P->m = m; P->list = order + filled; P->next = 0;
		pthread_mutex_init(&P->mu, NULL);
		P->device = pinned >= 0 ? pinned : gpemu_host_slot_device(s);
		for (int p = s; p < nlist; p += nslots) order[filled++] = list[p];
		P->n = (int)(order + filled - P->list);
	}
	for (int s = 0; s < nslots; s++) {
		/* slots of this call on the same physical device share its memory (GPEMU_DEVICES=0,0,0: three slots, one GPU) */
		int same = 0;
		for (int t = 0; t < nslots; t++) same += pools[t].device == pools[s].device;
		int c = want;
		if (!c) {
			const optstruct *o = m->pca_model_array[pools[s].list[0]]->options;
			const double need = 2.0 * gpemu_host_group_bytes(o->nmodel_points, 16);
			size_t fr = 0, tot = 0;
			c = 8;
			if (gpemu_device_memory(pools[s].device, &fr, &tot) == GPEMU_OK && fr > 0)
				while (c > 1 && (double)c * same * need > 0.9 * (double)fr) c--;
		}
		if (c > pools[s].n) c = pools[s].n;
		nthreads[s] = c;
		pools[s].share = c * same;
		total_threads += c;
	}
	if (total_threads == 1) {
		/* one component at a time on the caller's own thread, which stays as it is: unpinned, the search of a lone
		 * component deals its lock-step groups to EVERY device slot (estimate_thetas_threaded) */
		for (int p = 0; p < pools[0].n; p++) {
			modelstruct *c = m->pca_model_array[pools[0].list[p]];
			estimate_thetas_threaded(c, c->options);
		}
	} else {
		pthread_t *tid = (pthread_t *)calloc((size_t)total_threads, sizeof *tid);
		int t = 0;
		for (int s = 0; s < nslots; s++)
			for (int k = 0; k < nthreads[s]; k++, t++)
				if (pthread_create(&tid[t], NULL, component_main, &pools[s])) { perror("pthread_create"); gpemu_host_exit(EXIT_FAILURE); }
		for (t = 0; t < total_threads; t++)
			if (pthread_join(tid[t], NULL)) { perror("pthread_join"); gpemu_host_exit(EXIT_FAILURE); }
		free(tid);
	}
	for (int s = 0; s < nslots; s++) pthread_mutex_destroy(&pools[s].mu);
	free(pools); free(order); free(nthreads);
}

/* one process per GPU (ranks.c): rank r trains the components c = r, r + W, ...; the thetas of all components meet in ONE
 * all-gather (nthetas doubles per component, the shares padded to the same length); every rank then holds the whole model,
 * rank 0 writes it.  A single-output model has nothing to deal here: estimate_thetas_threaded deals its run list instead. */
static int g_components_over_ranks = 0;
int gpemu_host_components_over_ranks(void) { return g_components_over_ranks; }

static void estimate_multi_ranks(multi_modelstruct *m, FILE *outfp)
{
	const int world = gpemu_host_world_size(), rank = gpemu_host_rank();
	const int nthetas = (int)m->pca_model_array[0]->thetas->size;
	const int share = (m->nr + world - 1) / world;                  /* components per rank, padded */
	int *mine = (int *)malloc(sizeof(int) * (size_t)(share > 0 ? share : 1)), nmine = 0;
	for (int i = rank; i < m->nr; i += world) mine[nmine++] = i;
	g_components_over_ranks = 1;
	train_components(m, mine, nmine);
	g_components_over_ranks = 0;
	free(mine);
	double *send = (double *)calloc((size_t)share * nthetas, sizeof(double));
	double *recv = (double *)calloc((size_t)share * nthetas * world, sizeof(double));
	for (int j = 0, i = rank; i < m->nr; i += world, j++)
		for (int t = 0; t < nthetas; t++) send[(size_t)j * nthetas + t] = gsl_vector_get(m->pca_model_array[i]->thetas, t);
	gpemu_host_allgather(send, share * nthetas, recv);
	for (int i = 0; i < m->nr; i++) {
		const double *src = recv + ((size_t)(i % world) * share + (size_t)(i / world)) * nthetas;
		for (int t = 0; t < nthetas; t++) gsl_vector_set(m->pca_model_array[i]->thetas, t, src[t]);
	}
	free(send); free(recv);
	if (rank == 0) dump_multi_modelstruct(outfp, m);
}

void estimate_multi(multi_modelstruct *m, FILE *outfp)
{
	if (gpemu_host_world_size() > 1) {
		if (m->nr > 1) { estimate_multi_ranks(m, outfp); return; }
		/* one component: its run list is dealt to the ranks inside estimate_thetas_threaded; every rank returns the same thetas */
		estimate_thetas_threaded(m->pca_model_array[0], m->pca_model_array[0]->options);
		if (gpemu_host_rank() == 0) dump_multi_modelstruct(outfp, m);
		return;
	}
	int *all = (int *)malloc(sizeof(int) * (size_t)m->nr);
	for (int i = 0; i < m->nr; i++) all[i] = i;
	train_components(m, all, m->nr);
	free(all);
	dump_multi_modelstruct(outfp, m);
}

/* multivar_support.c:30-52 */
multi_emulator *alloc_multi_emulator(multi_modelstruct *m)
{
	multi_emulator *e = (multi_emulator *)malloc(sizeof(multi_emulator));
	e->nt = m->nt; e->nr = m->nr; e->nparams = m->nparams; e->nmodel_points = m->nmodel_points;
	e->nregression_fns = m->pca_model_array[0]->options->nregression_fns;
	e->nthetas = m->pca_model_array[0]->options->nthetas;
	e->model = m;
	e->emu_struct_array = (emulator_struct **)malloc(sizeof(emulator_struct *) * (size_t)e->nr);
	/* component i lives on device slot i mod S: emulate_points_multi starts all of them before it waits for the first.  The
	 * components that share a device are set up by ONE lock-step factorisation (gpemu_host_alloc_emulators) instead of the
	 * reference's one alloc_emulator_struct after the other: eight single-matrix chains are eight times the latency-bound
	 * panel chain, a batch of eight pays it once. */
	const int pinned = gpemu_host_thread_device_get();
	const int fill_cinverse = getenv("GPEMU_SKIP_CINVERSE") == NULL;
	modelstruct **models = (modelstruct **)malloc(sizeof(modelstruct *) * (size_t)e->nr);
	emulator_struct **made = (emulator_struct **)malloc(sizeof(emulator_struct *) * (size_t)e->nr);
	int *which = (int *)malloc(sizeof(int) * (size_t)e->nr);
	char *done = (char *)calloc((size_t)e->nr, 1);
	for (int first = 0; first < e->nr; first++) {
		if (done[first]) continue;
		const int dev = pinned >= 0 ? pinned : gpemu_host_slot_device(first);
		int n = 0;
		for (int i = first; i < e->nr; i++)              /* every component whose slot sits on this device */
			if (!done[i] && (pinned >= 0 || gpemu_host_slot_device(i) == dev)) { models[n] = m->pca_model_array[i]; which[n++] = i; done[i] = 1; }
		gpemu_host_thread_device(dev);
		if (fill_cinverse) {
			/* the reference's public emulator_struct.cinverse is wanted (library callers): every component is set up on its
			 * own -- the explicit N x N inverse comes out of a component's OWN factorisation workspace, and downloading and
			 * mirroring it dwarfs what a batch saves */
			for (int k = 0; k < n; k++) made[k] = gpemu_host_alloc_emulator(models[k], 1);
		} else {
			for (int b0 = 0; b0 < n; b0 += 16) {           /* (workspace: 16 x (2 Np + 64) x Np x 8 bytes per call) */
				const int nb = n - b0 < 16 ? n - b0 : 16;
				gpemu_host_alloc_emulators(models + b0, nb, 0, made + b0);
			}
		}
		for (int k = 0; k < n; k++) e->emu_struct_array[which[k]] = made[k];
	}
	gpemu_host_thread_device(pinned);
	free(which);
	free(models); free(made); free(done);
	return e;
}

void free_multi_emulator(multi_emulator *e)
{
	for (int i = 0; i < e->nr; i++) free_emulator_struct(e->emu_struct_array[i]);
	free(e->emu_struct_array);
	free_multimodelstruct(e->model);
	free(e);
}

/* The PCA -> observable rule of the reference (multivar_support.c:118-157), written once for every entry below:
 *   out[q][t][j] = (add_mean && j == 0 ? training_mean[t] : 0) + sum_c F[t][c] * in[q][c][j],   q < nrows, j < width
 * with F = evecs * sqrt(evals) (squared = 0: means and their gradients) or evecs^2 * evals (squared = 1: variances, their
 * gradients, covariances).  This is the summation order of every observable-space number the library returns: the factor is
 * formed first and then multiplied by the input element, the sum runs over c in index order from 0.0, and the training mean
 * is added to the finished sum.  j is the innermost loop, so a component-major [c][M^2] covariance buffer (nrows = 1,
 * width = M^2) is streamed with unit stride. */
void gpemu_host_backproject(const multi_modelstruct *m, int squared, int add_mean, size_t nrows, size_t width,
                            const double *in, double *out)
{
	const size_t nt = (size_t)m->nt, nr = (size_t)m->nr;
	for (size_t q = 0; q < nrows; q++)
		for (size_t t = 0; t < nt; t++) {
			double *o = out + (q * nt + t) * width;
			for (size_t j = 0; j < width; j++) o[j] = 0.0;
			for (size_t c = 0; c < nr; c++) {
				const double u = gsl_matrix_get(m->pca_evecs_r, t, c), lam = gsl_vector_get(m->pca_evals_r, c);
				const double f = squared ? pow(u, 2.0) * lam : u * sqrt(lam);
				const double *ic = in + (q * nr + c) * width;
				for (size_t j = 0; j < width; j++) o[j] += f * ic[j];
			}
			if (add_mean && width) o[0] = gsl_vector_get(m->training_mean, t) + o[0];
		}
}

static double *doubles(size_t n) { return (double *)malloc(sizeof(double) * n); }

/* component c's np x w result into the [q][c][w] layout of the PCA-space outputs, which the back-projection reads */
static void place_component(double *all, const double *one, size_t np, size_t nr, size_t c, size_t w)
{
	for (size_t q = 0; q < np; q++) memcpy(all + (q * nr + c) * w, one + q * w, sizeof(double) * w);
}

/* np x nr x w PCA-space results to the caller: as they are, or np x nt x w through the back-projection */
static void deliver(const multi_emulator *emu, int pca_space, int squared, int add_mean, size_t np, size_t w, const double *in, double *out)
{
	if (pca_space) memcpy(out, in, sizeof(double) * np * (size_t)emu->nr * w);
	else gpemu_host_backproject(emu->model, squared, add_mean, np, w, in, out);
}

void emulate_points_multi(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *var_out)
{
	const size_t np = points->size1, nr = (size_t)emu->nr;
	double *mp = doubles(np * nr), *vp = doubles(np * nr), *mc = doubles(np), *vc = doubles(np);
	/* the nr scalar emulators are independent (multivar_support.c:116 loops over them): each has its own device
	 * context, so all of them are started before the first result is waited for */
	for (size_t c = 0; c < nr; c++) emulate_points_enqueue(emu->emu_struct_array[c], points);
	for (size_t c = 0; c < nr; c++) {
		emulate_points_collect(emu->emu_struct_array[c], (int)np, mc, vc);
		place_component(mp, mc, np, nr, c, 1);
		place_component(vp, vc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	deliver(emu, pca_space, 1, 0, np, 1, vp, var_out);
	free(mp); free(vp); free(mc); free(vc);
}

/* the means alone: every component through its mean-only sweep (all enqueued, then collected, as above); observable space by
 * the mean half of the rule, which needs no variances */
void emulate_points_multi_mean(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out)
{
	const size_t np = points->size1, nr = (size_t)emu->nr;
	double *mp = doubles(np * nr), *mc = doubles(np);
	for (size_t c = 0; c < nr; c++) emulate_points_mean_enqueue(emu->emu_struct_array[c], points);
	for (size_t c = 0; c < nr; c++) {
		emulate_points_mean_collect(emu->emu_struct_array[c], (int)np, mc);
		place_component(mp, mc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	free(mp); free(mc);
}

/* means and their gradients with respect to the query point: every component through its fused sweep (all enqueued, then
 * collected); in observable space the gradient takes the mean's factor without the training mean, which is a constant */
void emulate_points_multi_mean_grad(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *grad_out)
{
	const size_t np = points->size1, nr = (size_t)emu->nr, d = points->size2;
	double *mp = doubles(np * nr), *mc = doubles(np), *gp = doubles(np * nr * d), *gc = doubles(np * d);
	for (size_t c = 0; c < nr; c++) emulate_points_mean_grad_enqueue(emu->emu_struct_array[c], points);
	for (size_t c = 0; c < nr; c++) {
		emulate_points_mean_grad_collect(emu->emu_struct_array[c], (int)np, mc, gc);
		place_component(mp, mc, np, nr, c, 1);
		place_component(gp, gc, np, nr, c, d);
	}
	if (mean_out) deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	deliver(emu, pca_space, 0, 0, np, d, gp, grad_out);
	free(mp); free(mc); free(gp); free(gc);
}

/* means, variances and the gradients of both: every component's variance-gradient batch is started before the first is
 * collected (its mean-gradient sweep, when asked for, runs at its collect); in observable space the mean and its gradient
 * take the rule's mean factor, the variance and its gradient the squared one */
void emulate_points_multi_grad(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *var_out,
                               double *grad_mean_out, double *grad_var_out)
{
	const size_t np = points->size1, nr = (size_t)emu->nr, d = points->size2;
	if (!mean_out && !var_out && !grad_mean_out && !grad_var_out) gpemu_host_fatal("emulate_points_multi_grad: every output is NULL\n");
	if (!var_out && !grad_var_out) {                     /* no variance asked for: the mean-gradient sweeps alone */
		double *g = grad_mean_out ? grad_mean_out : doubles(np * (size_t)(pca_space ? emu->nr : emu->nt) * d);
		emulate_points_multi_mean_grad(emu, points, pca_space, mean_out, g);
		if (!grad_mean_out) free(g);
		return;
	}
	double *mp = doubles(np * nr), *vp = doubles(np * nr), *gm = doubles(np * nr * d), *gv = doubles(np * nr * d);
	double *mc = doubles(np), *vc = doubles(np), *gmc = doubles(np * d), *gvc = doubles(np * d);
	for (size_t c = 0; c < nr; c++) emulate_points_grad_enqueue(emu->emu_struct_array[c], points);
	for (size_t c = 0; c < nr; c++) {
		emulate_points_grad_collect(emu->emu_struct_array[c], (int)np, mc, vc, grad_mean_out ? gmc : NULL, gvc);
		place_component(mp, mc, np, nr, c, 1);
		place_component(vp, vc, np, nr, c, 1);
		if (grad_mean_out) place_component(gm, gmc, np, nr, c, d);
		place_component(gv, gvc, np, nr, c, d);
	}
	if (mean_out) deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	if (var_out) deliver(emu, pca_space, 1, 0, np, 1, vp, var_out);
	if (grad_mean_out) deliver(emu, pca_space, 0, 0, np, d, gm, grad_mean_out);
	if (grad_var_out) deliver(emu, pca_space, 1, 0, np, d, gv, grad_var_out);
	free(mp); free(vp); free(gm); free(gv); free(mc); free(vc); free(gmc); free(gvc);
}

/* the joint posterior covariance between the query points, per output (libemu.h): every component's gpemu_predict_cov_dev is
 * enqueued on its own stream before the first is collected.  The component matrices land component-major, [c][np x np]: in PCA
 * space that is the output; in observable space it is ONE row of width np x np for the squared rule, every element alike */
void emulate_points_multi_cov(multi_emulator *emu, gsl_matrix *points, int pca_space, double *mean_out, double *cov_out)
{
	const size_t np = points->size1, nr = (size_t)emu->nr, mm = np * np;
	if (!cov_out) gpemu_host_fatal("emulate_points_multi_cov: cov_out is NULL\n");
	double *mp = doubles(np * nr), *mc = doubles(np);
	double *cp = pca_space ? cov_out : doubles(mm * nr);
	void **dev = (void **)malloc(sizeof(void *) * nr);
	for (size_t c = 0; c < nr; c++) emulate_points_cov_enqueue(emu->emu_struct_array[c], points, &dev[c]);
	for (size_t c = 0; c < nr; c++) {
		emulate_points_cov_collect(emu->emu_struct_array[c], dev[c], (int)np, mc, cp + mm * c);
		place_component(mp, mc, np, nr, c, 1);
	}
	if (!pca_space) {
		gpemu_host_backproject(emu->model, 1, 0, 1, mm, cp, cov_out);
		free(cp);
	}
	if (mean_out) deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	free(mp); free(mc); free(dev);
}

/* Validation on a held-out campaign (libemu.h).  The observations Y (np x nt, observable space) go to PCA space by the
 * arithmetic gen_pca_decomp builds pca_zmatrix with -- z[c][p] = (sum_t (Y[p][t] - training_mean[t]) evecs[t][c]) * (1 / sqrt(evals[c])),
 * t in index order from 0.0 --, component-major, one row of np per component; then every component's factor call is enqueued
 * on its own stream before the first is collected.  The components are independent emulators, so the joint log density of
 * the projected observations is the sum of theirs. */
void gpemu_host_project_observations(const multi_modelstruct *m, size_t np, const double *Y, double *z)
{
	const size_t nt = (size_t)m->nt, nr = (size_t)m->nr;
	for (size_t p = 0; p < np; p++)
		for (size_t c = 0; c < nr; c++) {
			double s = 0.0;
			for (size_t t = 0; t < nt; t++) s += (Y[p * nt + t] - gsl_vector_get(m->training_mean, t)) * gsl_matrix_get(m->pca_evecs_r, t, c);
			z[c * np + p] = s * (1.0 / sqrt(gsl_vector_get(m->pca_evals_r, c)));
		}
}

/* ---- implausibility and calibration likelihood against observations (libemu.h; gpemu_calib_* in gpemu.h) */
struct gpemu_observations { int nt, nr; double c_perp, logdet_S, logdet_G; };

gpemu_observations *alloc_observations(multi_modelstruct *m, const double *z, const double *sd, const double *cov, const double *rel)
{
	const size_t nt = (size_t)m->nt, nr = (size_t)m->nr;
	if (!z || (sd == NULL) == (cov == NULL)) gpemu_host_fatal("alloc_observations: z and exactly one of sd and cov are needed\n");
	if (m->nr > GPEMU_CALIB_MAX_R || m->nt > GPEMU_CALIB_MAX_NT)
		gpemu_host_fatal("alloc_observations: nr = %d, nt = %d: more than %d components or %d outputs is not built\n", m->nr, m->nt,
		                 GPEMU_CALIB_MAX_R, GPEMU_CALIB_MAX_NT);
	double *A = doubles(nt * nr), *ybar = doubles(nt), mhat[GPEMU_CALIB_MAX_R], sigz[GPEMU_CALIB_MAX_R * GPEMU_CALIB_MAX_R], consts[3];
	for (size_t t = 0; t < nt; t++) {
		ybar[t] = gsl_vector_get(m->training_mean, t);
		for (size_t c = 0; c < nr; c++) A[t * nr + c] = gsl_matrix_get(m->pca_evecs_r, t, c) * sqrt(gsl_vector_get(m->pca_evals_r, c));
	}
	int info = 0;
	const int rc = gpemu_calib_project(m->nt, m->nr, ybar, A, z, cov, sd, mhat, sigz, consts, &info);
	if (rc == GPEMU_ERR_NOT_PD)
		gpemu_host_fatal("alloc_observations: the observation covariance, or A^T S^-1 A, is not positive definite (pivot %d)\n", info);
	if (rc) gpemu_host_fatal("alloc_observations: non-finite input or a standard deviation <= 0\n");
	for (size_t t = 0; rel && t < nt; t++)
		if (!(rel[t] >= 0.0) || !isfinite(rel[t])) gpemu_host_fatal("alloc_observations: rel[%zu] must be finite and >= 0\n", t);
	gpemu_observations *obs = (gpemu_observations *)malloc(sizeof *obs);
	obs->nt = m->nt; obs->nr = m->nr;
	obs->c_perp = consts[0]; obs->logdet_S = consts[1]; obs->logdet_G = consts[2];
	gpemu_host_calib_setup(obs, m->nt, m->nr, ybar, A, z, cov, sd, rel);
	free(A); free(ybar);
	return obs;
}

void free_observations(gpemu_observations *obs)
{
	if (!obs) return;
	gpemu_host_release(obs);
	free(obs);
}

void gpemu_host_observations_misfit(const gpemu_observations *obs, double *c_perp, int *dof)
{
	if (c_perp) *c_perp = obs->c_perp;
	if (dof) *dof = obs->nt - obs->nr;
}

/* x with erfc(x / sqrt 2) = sig, that is qnorm(1 - sig / 2): erfc is monotone, so bisection on [0, 40] to the last bit */
double gpemu_host_confidence_to_rel(double sig)
{
	if (!(sig > 0.0 && sig < 1.0)) return NAN;
	double lo = 0.0, hi = 40.0;
	for (int it = 0; it < 200 && lo < hi; it++) {
		const double mid = 0.5 * (lo + hi);
		if (mid <= lo || mid >= hi) break;
		if (erfc(mid * M_SQRT1_2) > sig) lo = mid; else hi = mid;
	}
	return sig / (0.5 * (lo + hi));
}

#define CALIB_HOST_BLOCK 262144
static void calib_points(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, int select, double cut_chi2, int level,
                         double cut_I, double *stat_out, int *worst_out, int *idx_out, int *nkeep, const char *who)
{
	if (!emu || !obs || !points || !stat_out) gpemu_host_fatal("%s: a NULL argument\n", who);
	if (obs->nr != emu->nr || obs->nt != emu->nt) gpemu_host_fatal("%s: the observation set belongs to another model\n", who);
	if (select && (!idx_out || !nkeep || level < 1 || level > 3 || cut_chi2 != cut_chi2 || cut_I != cut_I))
		gpemu_host_fatal("%s: idx_out, nkeep, a level in 1 .. 3 and cuts that are not NaN are needed\n", who);
	const size_t np = points->size1, d = points->size2;
	size_t kept = 0;
	double *q = doubles((np < CALIB_HOST_BLOCK ? np : CALIB_HOST_BLOCK) * d + 1);
	for (size_t p0 = 0; p0 < np; p0 += CALIB_HOST_BLOCK) {
		const size_t nb = np - p0 < CALIB_HOST_BLOCK ? np - p0 : CALIB_HOST_BLOCK;
		for (size_t p = 0; p < nb; p++)
			for (size_t j = 0; j < d; j++) q[p * d + j] = gsl_matrix_get(points, p0 + p, j);
		if (!select) {
			gpemu_host_calib_block(obs, emu->emu_struct_array, emu->nr, (int)nb, (int)d, q, 0, 0.0, 1, 0.0, stat_out + p0 * 5,
			                       worst_out ? worst_out + p0 : NULL, NULL, NULL);
			continue;
		}
		int k = 0;
		gpemu_host_calib_block(obs, emu->emu_struct_array, emu->nr, (int)nb, (int)d, q, 1, cut_chi2, level, cut_I, stat_out + kept * 5,
		                       worst_out ? worst_out + kept : NULL, idx_out + kept, &k);
		for (int i = 0; i < k; i++) idx_out[kept + (size_t)i] += (int)p0;
		kept += (size_t)k;
	}
	free(q);
	if (nkeep) *nkeep = (int)kept;
}

void emulate_points_multi_implausibility(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double *stat_out, int *worst_out)
{
	calib_points(emu, obs, points, 0, 0.0, 1, 0.0, stat_out, worst_out, NULL, NULL, "emulate_points_multi_implausibility");
}

void emulate_points_multi_nonimplausible(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double cut_chi2, int level,
                                         double cut_I, int *idx_out, double *stat_out, int *nkeep)
{
	calib_points(emu, obs, points, 1, cut_chi2, level, cut_I, stat_out, NULL, idx_out, nkeep, "emulate_points_multi_nonimplausible");
}

void emulate_points_multi_nonimplausible_worst(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double cut_chi2, int level,
                                               double cut_I, int *idx_out, double *stat_out, int *worst_out, int *nkeep)
{
	calib_points(emu, obs, points, 1, cut_chi2, level, cut_I, stat_out, worst_out, idx_out, nkeep, "emulate_points_multi_nonimplausible");
}

/* the gradient of the joint log density (and of chi2) with respect to the points' coordinates (libemu.h): blocks of
 * CALIB_GRAD_HOST_BLOCK points through gpemu_host_calib_grad_block */
#define CALIB_GRAD_HOST_BLOCK 16384
void emulate_points_multi_logpdf_grad(multi_emulator *emu, gpemu_observations *obs, gsl_matrix *points, double *stat_out,
                                      double *grad_logpdf_out, double *grad_chi2_out)
{
	static const char who[] = "emulate_points_multi_logpdf_grad";
	if (!emu || !obs || !points || !grad_logpdf_out) gpemu_host_fatal("%s: a NULL argument\n", who);
	if (obs->nr != emu->nr || obs->nt != emu->nt) gpemu_host_fatal("%s: the observation set belongs to another model\n", who);
	const size_t np = points->size1, d = points->size2;
	double *q = doubles((np < CALIB_GRAD_HOST_BLOCK ? np : CALIB_GRAD_HOST_BLOCK) * d + 1);
	for (size_t p0 = 0; p0 < np; p0 += CALIB_GRAD_HOST_BLOCK) {
		const size_t nb = np - p0 < CALIB_GRAD_HOST_BLOCK ? np - p0 : CALIB_GRAD_HOST_BLOCK;
		for (size_t p = 0; p < nb; p++)
			for (size_t j = 0; j < d; j++) q[p * d + j] = gsl_matrix_get(points, p0 + p, j);
		gpemu_host_calib_grad_block(obs, emu->emu_struct_array, emu->nr, (int)nb, (int)d, q, stat_out ? stat_out + p0 * 5 : NULL,
		                            grad_logpdf_out + p0 * d, grad_chi2_out ? grad_chi2_out + p0 * d : NULL);
	}
	free(q);
}

void emulate_points_multi_holdout(multi_emulator *emu, gsl_matrix *points, const double *Y, const double *noise_pca, double *mean_out,
                                  double *var_out, double *werr_out, double *maha_out, double *logdet_out, double *logpdf_out,
                                  double *logpdf_sum)
{
	const size_t np = points->size1, nr = (size_t)emu->nr;
	const int nobs = Y ? 1 : 0;
	double *z = Y ? doubles(nr * np) : NULL;
	double *mp = doubles(np * nr), *vp = doubles(np * nr), *wp = doubles(np * nr), *mc = doubles(np), *vc = doubles(np), *wc = doubles(np);
	void **dev = (void **)malloc(sizeof(void *) * nr);
	if (Y) gpemu_host_project_observations(emu->model, np, Y, z);
	for (size_t c = 0; c < nr; c++)
		emulate_points_holdout_enqueue(emu->emu_struct_array[c], points, Y ? z + c * np : NULL, noise_pca ? noise_pca + c * np : NULL, &dev[c]);
	double sum = 0.0;
	for (size_t c = 0; c < nr; c++) {
		double maha = 0.0, logdet = 0.0, logpdf = 0.0;
		emulate_points_holdout_collect(emu->emu_struct_array[c], dev[c], (int)np, nobs, mc, vc, wc, &maha, &logdet, &logpdf);
		place_component(mp, mc, np, nr, c, 1);
		place_component(vp, vc, np, nr, c, 1);
		if (nobs) place_component(wp, wc, np, nr, c, 1);
		if (maha_out && nobs) maha_out[c] = maha;
		if (logdet_out) logdet_out[c] = logdet;
		if (logpdf_out && nobs) logpdf_out[c] = logpdf;
		sum += logpdf;
	}
	if (mean_out) memcpy(mean_out, mp, sizeof(double) * np * nr);
	if (var_out) memcpy(var_out, vp, sizeof(double) * np * nr);
	if (werr_out && nobs) memcpy(werr_out, wp, sizeof(double) * np * nr);
	if (logpdf_sum && nobs) *logpdf_sum = sum;
	free(z); free(mp); free(vp); free(wp); free(mc); free(vc); free(wc); free(dev);
}

/* joint draws at the points of the last emulate_points_multi_holdout: component c draws from its own resident factor with its
 * own normals z[c] (ndraw x np); the results land [s][p][c], which is the PCA-space output, and go to observable space through
 * the mean half of the rule, training mean added */
void emulate_points_multi_draw(multi_emulator *emu, int pca_space, int npoints, int ndraw, const double *z, double *out)
{
	const size_t np = (size_t)npoints, nd = (size_t)ndraw, nr = (size_t)emu->nr;
	double *dp = doubles(nd * np * nr), *dc = doubles(nd * np);
	for (size_t c = 0; c < nr; c++) {
		emulate_points_draw(emu->emu_struct_array[c], ndraw, z + c * nd * np, dc);
		place_component(dp, dc, nd * np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, nd * np, 1, dp, out);
	free(dp); free(dc);
}

/* leave-one-out at every training point: the components are independent contexts, so all are started before the first is
 * waited for, as above; component results are N x nr in design order, then the same back-projection */
void emulate_loo_multi(multi_emulator *emu, int pca_space, double *mean_out, double *var_out)
{
	const size_t np = (size_t)emu->nmodel_points, nr = (size_t)emu->nr;
	double *mp = doubles(np * nr), *vp = doubles(np * nr), *mc = doubles(np), *vc = doubles(np);
	void **dev = (void **)malloc(sizeof(void *) * nr);
	for (size_t c = 0; c < nr; c++) emulate_loo_enqueue(emu->emu_struct_array[c], &dev[c]);
	for (size_t c = 0; c < nr; c++) {
		emulate_loo_collect(emu->emu_struct_array[c], dev[c], mc, vc);
		place_component(mp, mc, np, nr, c, 1);
		place_component(vp, vc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	deliver(emu, pca_space, 1, 0, np, 1, vp, var_out);
	free(mp); free(vp); free(mc); free(vc); free(dev);
}

/* K-fold / leave-group-out validation, the same groups for every component: started and collected as above; the per-group
 * diagnostics stay in PCA space, component-major */
void emulate_lgo_multi(multi_emulator *emu, int pca_space, int ngroups, const int *group, double *mean_out, double *var_out,
                       double *maha_out, double *logpdf_out)
{
	const size_t np = (size_t)emu->nmodel_points, nr = (size_t)emu->nr, ng = (size_t)(ngroups > 0 ? ngroups : 0);
	double *mp = doubles(np * nr), *vp = doubles(np * nr), *mc = doubles(np), *vc = doubles(np);
	void **dev = (void **)malloc(sizeof(void *) * nr);
	for (size_t c = 0; c < nr; c++) emulate_lgo_enqueue(emu->emu_struct_array[c], ngroups, group, &dev[c]);
	for (size_t c = 0; c < nr; c++) {
		emulate_lgo_collect(emu->emu_struct_array[c], dev[c], ngroups, mc, vc, NULL, maha_out ? maha_out + c * ng : NULL,
		                    logpdf_out ? logpdf_out + c * ng : NULL);
		place_component(mp, mc, np, nr, c, 1);
		place_component(vp, vc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, mp, mean_out);
	deliver(emu, pca_space, 1, 0, np, 1, vp, var_out);
	free(mp); free(vp); free(mc); free(vc); free(dev);
}

/* Sensitivity analysis of every output over the box [lo, hi] (libemu.h).  PCA space: component c against itself, nr calls.
 * Observable space: y_t = training_mean[t] + sum_c B_tc m_c, B_tc = evecs[t][c] sqrt(evals[c]).  The components are functions of
 * the SAME inputs, so under the input measure they are correlated and every conditional variance is the full quadratic form
 *   Var_u(y_t) = sum_{c,c'} B_tc B_tc' cov_u(c, c')
 * over all pairs: nr (nr + 1) / 2 device calls on two contexts each (cov_u is symmetric in the pair), all enqueued before the
 * first is collected.  gpemu_host_backproject's squared rule, sum_c B_tc^2 var_c, is NOT used here: it is right for the
 * emulator's posterior variance, where the components are independent random functions, and would drop every cross term of
 * this one, where they are fixed functions of a random input. */
void emulate_sensitivity_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *e0_out, double *var_out,
                               double *first_out, double *total_out)
{
	const size_t nr = (size_t)emu->nr, nt = (size_t)emu->nt, d = (size_t)emu->nparams;
	const size_t npair = pca_space ? nr : nr * (nr + 1) / 2, w = 1 + 2 * d;
	void **dev = (void **)malloc(sizeof(void *) * npair);
	double *cv = doubles(npair * w), *e0 = doubles(nr), both[2];
	size_t k = 0;
	for (size_t c = 0; c < nr; c++)
		for (size_t c2 = c; c2 < (pca_space ? c + 1 : nr); c2++)
			emulate_sensitivity_enqueue(emu->emu_struct_array[c], emu->emu_struct_array[c2], lo, hi, &dev[k++]);
	k = 0;
	for (size_t c = 0; c < nr; c++)
		for (size_t c2 = c; c2 < (pca_space ? c + 1 : nr); c2++, k++) {
			/* row k: cov_all, cov_first[d], cov_rest[d] of the pair */
			emulate_sensitivity_collect(emu->emu_struct_array[c], dev[k], both, cv + k * w, cv + k * w + 1, cv + k * w + 1 + d);
			if (c2 == c) e0[c] = both[0];
		}
	if (pca_space) {
		for (size_t c = 0; c < nr; c++) {
			e0_out[c] = e0[c];
			var_out[c] = cv[c * w];
			for (size_t j = 0; j < d; j++) {
				first_out[c * d + j] = cv[c * w + 1 + j];
				total_out[c * d + j] = cv[c * w] - cv[c * w + 1 + d + j];
			}
		}
	} else {
		double *acc = doubles(w);
		for (size_t t = 0; t < nt; t++) {
			for (size_t i = 0; i < w; i++) acc[i] = 0.0;
			double m = 0.0;
			k = 0;
			for (size_t c = 0; c < nr; c++) {
				const double bc = gsl_matrix_get(emu->model->pca_evecs_r, t, c) * sqrt(gsl_vector_get(emu->model->pca_evals_r, c));
				m += bc * e0[c];
				for (size_t c2 = c; c2 < nr; c2++, k++) {
					const double b2 = gsl_matrix_get(emu->model->pca_evecs_r, t, c2) * sqrt(gsl_vector_get(emu->model->pca_evals_r, c2));
					const double f = (c2 == c ? 1.0 : 2.0) * bc * b2;
					for (size_t i = 0; i < w; i++) acc[i] += f * cv[k * w + i];
				}
			}
			e0_out[t] = gsl_vector_get(emu->model->training_mean, t) + m;
			var_out[t] = acc[0];
			for (size_t j = 0; j < d; j++) {
				first_out[t * d + j] = acc[1 + j];
				total_out[t * d + j] = acc[0] - acc[1 + d + j];
			}
		}
		free(acc);
	}
	free(dev); free(cv); free(e0);
}

/* the input measure of every sensitivity call on emu from now on: every component gets the same kinds (libemu.h) */
void emulate_sensitivity_measure_multi(multi_emulator *emu, const int *kind)
{
	for (size_t c = 0; c < (size_t)emu->nr; c++) emulate_sensitivity_measure(emu->emu_struct_array[c], kind);
}

/* main-effect curves of every output: the components one after the other (gpemu_sens_main waits for its result), then the mean
 * half of the rule -- a conditional mean is linear in the components -- with the training mean added */
void emulate_main_effects_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int ngrid, const double *grid,
                                double *e0_out, double *main_out)
{
	const size_t nr = (size_t)emu->nr, np = (size_t)emu->nparams * (size_t)(ngrid > 0 ? ngrid : 0);
	double *mp = doubles(np * nr), *mc = doubles(np), *ep = doubles(nr);
	for (size_t c = 0; c < nr; c++) {
		emulate_main_effects(emu->emu_struct_array[c], lo, hi, ngrid, grid, &ep[c], mc);
		place_component(mp, mc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, mp, main_out);
	deliver(emu, pca_space, 0, 1, 1, 1, ep, e0_out);
	free(mp); free(mc); free(ep);
}

/* The emulator-uncertainty terms of every output (libemu.h).  The plug-in part comes from emulate_sensitivity_multi, cross terms
 * and all.  The S terms of the components go through the SQUARED rule: they are posterior variances and the components are
 * independent a posteriori, S_u(y_t) = sum_c B_tc^2 S_u^c. */
void emulate_sensitivity_uncertainty_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *var_e0_out,
                                           double *imse_out, double *evar_out, double *efirst_out, double *etotal_out)
{
	const size_t nr = (size_t)emu->nr, d = (size_t)emu->nparams, w = 2 + 2 * d, nout = pca_space ? nr : (size_t)emu->nt;
	double *sc = doubles(nr * w), *so = doubles(nout * w), *e0 = doubles(nout), *var = doubles(nout);
	emulate_sensitivity_multi(emu, pca_space, lo, hi, e0, var, efirst_out, etotal_out);
	for (size_t c = 0; c < nr; c++) emulate_sensitivity_post(emu->emu_struct_array[c], lo, hi, sc + c * w);
	deliver(emu, pca_space, 1, 0, 1, w, sc, so);
	for (size_t t = 0; t < nout; t++) {
		const double *s = so + t * w;
		var_e0_out[t] = s[0];
		imse_out[t] = s[1];
		evar_out[t] = var[t] + s[1] - s[0];
		for (size_t j = 0; j < d; j++) {
			efirst_out[t * d + j] += s[2 + j] - s[0];
			etotal_out[t * d + j] += s[1] - s[2 + d + j];
		}
	}
	free(sc); free(so); free(e0); free(var);
}

/* the curves by the mean half of the rule, their posterior variances by the squared half, then the square root */
void emulate_main_effects_band_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int ngrid, const double *grid,
                                     double *e0_out, double *main_out, double *sd_out)
{
	const size_t nr = (size_t)emu->nr, np = (size_t)emu->nparams * (size_t)(ngrid > 0 ? ngrid : 0);
	const size_t nout = pca_space ? nr : (size_t)emu->nt;
	double *mp = doubles(np * nr), *vp = doubles(np * nr), *mc = doubles(np), *vc = doubles(np), *ep = doubles(nr);
	for (size_t c = 0; c < nr; c++) {
		emulate_main_effects_var(emu->emu_struct_array[c], lo, hi, ngrid, grid, &ep[c], mc, vc, NULL);
		place_component(mp, mc, np, nr, c, 1);
		place_component(vp, vc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, mp, main_out);
	deliver(emu, pca_space, 1, 0, np, 1, vp, sd_out);
	deliver(emu, pca_space, 0, 1, 1, 1, ep, e0_out);
	for (size_t i = 0; i < np * nout; i++) sd_out[i] = sqrt(sd_out[i] > 0.0 ? sd_out[i] : 0.0);
	free(mp); free(vp); free(mc); free(vc); free(ep);
}

/* The expected drop of every output's IMSE by one more run at each candidate (libemu.h): the components one after the other
 * (gpemu_design_gain waits for its result), then the squared half of the rule -- a run observes every component, and the
 * components are independent a posteriori. */
void emulate_design_gain_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int npoints, const double *points,
                               double *gain_out, double *total_out)
{
	const size_t nr = (size_t)emu->nr, np = (size_t)(npoints > 0 ? npoints : 0), nout = pca_space ? nr : (size_t)emu->nt;
	double *gp = doubles((np ? np : 1) * nr), *gc = doubles(np ? np : 1);
	for (size_t c = 0; c < nr; c++) {
		emulate_design_gain(emu->emu_struct_array[c], lo, hi, npoints, points, gc, NULL, NULL);
		place_component(gp, gc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 1, 0, np, 1, gp, gain_out);
	for (size_t q = 0; total_out && q < np; q++) {
		double s = 0.0;
		for (size_t t = 0; t < nout; t++) s += gain_out[q * nout + t];
		total_out[q] = s;
	}
	free(gp); free(gc);
}

/* The same over a weighted set of target points (libemu.h): the targets to every component, the components one after the other,
 * then the squared half of the rule for the gains and for the target variance.  A component's targets are released once its gains are
 * back. */
void emulate_design_target_gain_multi(multi_emulator *emu, int pca_space, int ntargets, const double *targets, const double *weight,
                                      int npoints, const double *points, double *gain_out, double *total_out, double *target_var_out)
{
	const size_t nr = (size_t)emu->nr, np = (size_t)(npoints > 0 ? npoints : 0), nout = pca_space ? nr : (size_t)emu->nt;
	double *gp = doubles((np ? np : 1) * nr), *gc = doubles(np ? np : 1), *tv = doubles(nr);
	for (size_t c = 0; c < nr; c++) {
		emulate_design_target_set(emu->emu_struct_array[c], ntargets, targets, weight, &tv[c], NULL);
		emulate_design_target_gain(emu->emu_struct_array[c], npoints, points, gc, NULL, NULL);
		emulate_design_target_release(emu->emu_struct_array[c]);       /* (the store is gigabytes at the limits: not kept per component) */
		place_component(gp, gc, np, nr, c, 1);
	}
	deliver(emu, pca_space, 1, 0, np, 1, gp, gain_out);
	if (target_var_out) deliver(emu, pca_space, 1, 0, 1, 1, tv, target_var_out);
	for (size_t q = 0; total_out && q < np; q++) {
		double s = 0.0;
		for (size_t t = 0; t < nout; t++) s += gain_out[q * nout + t];
		total_out[q] = s;
	}
	free(gp); free(gc); free(tv);
}

/* A greedy batch of runs (libemu.h).  The weights are what total_out above sums: the squared rule applied to the unit vectors of
 * the components gives B_tc^2, and weight_c is its sum over the outputs. */
void emulate_design_batch_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int npoints, const double *points,
                                int nbatch, int *pick_out, double *gain_out)
{
	const size_t nr = (size_t)emu->nr, nout = pca_space ? nr : (size_t)emu->nt;
	double *unit = doubles(nr * nr), *sq = doubles(nr * nout), *weight = doubles(nr);
	for (size_t i = 0; i < nr * nr; i++) unit[i] = i / nr == i % nr ? 1.0 : 0.0;
	deliver(emu, pca_space, 1, 0, nr, 1, unit, sq);
	for (size_t c = 0; c < nr; c++) {
		double s = 0.0;
		for (size_t t = 0; t < nout; t++) s += sq[c * nout + t];
		weight[c] = s;
	}
	emulate_design_batch_components(emu->emu_struct_array, (int)nr, weight, lo, hi, npoints, points, nbatch, pick_out, gain_out);
	free(unit); free(sq); free(weight);
}

/* Second order for every output (libemu.h): vpair_out[t * npairs + p] = V_jk of output t, inter_out the interaction variances
 * V_jk - V_j - V_k.  As emulate_sensitivity_multi: in observable space the full quadratic form over all pairs of components,
 *   V_jk(y_t) = sum_{c,c'} B_tc B_tc' cov_pair(c, c'),
 * every pair of components started before the first is collected; V_j and V_k from emulate_sensitivity_multi. */
void emulate_sensitivity_pairs_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *vpair_out,
                                     double *inter_out)
{
	const size_t nr = (size_t)emu->nr, nt = (size_t)emu->nt, d = (size_t)emu->nparams, w = d * (d ? d - 1 : 0) / 2;
	const size_t ncomp = pca_space ? nr : nr * (nr + 1) / 2, nout = pca_space ? nr : nt;
	void **dev = (void **)malloc(sizeof(void *) * ncomp);
	double *cv = doubles(ncomp * (w ? w : 1));
	size_t k = 0;
	for (size_t c = 0; c < nr; c++)
		for (size_t c2 = c; c2 < (pca_space ? c + 1 : nr); c2++)
			emulate_sensitivity_pairs_enqueue(emu->emu_struct_array[c], emu->emu_struct_array[c2], lo, hi, &dev[k++]);
	k = 0;
	for (size_t c = 0; c < nr; c++)
		for (size_t c2 = c; c2 < (pca_space ? c + 1 : nr); c2++, k++)
			emulate_sensitivity_pairs_collect(emu->emu_struct_array[c], dev[k], cv + k * w);
	if (pca_space) memcpy(vpair_out, cv, sizeof(double) * nr * w);
	else
		for (size_t t = 0; t < nt; t++) {
			double *acc = vpair_out + t * w;
			for (size_t i = 0; i < w; i++) acc[i] = 0.0;
			k = 0;
			for (size_t c = 0; c < nr; c++) {
				const double bc = gsl_matrix_get(emu->model->pca_evecs_r, t, c) * sqrt(gsl_vector_get(emu->model->pca_evals_r, c));
				for (size_t c2 = c; c2 < nr; c2++, k++) {
					const double b2 = gsl_matrix_get(emu->model->pca_evecs_r, t, c2) * sqrt(gsl_vector_get(emu->model->pca_evals_r, c2));
					const double f = (c2 == c ? 1.0 : 2.0) * bc * b2;
					for (size_t i = 0; i < w; i++) acc[i] += f * cv[k * w + i];
				}
			}
		}
	double *e0 = doubles(nout), *var = doubles(nout), *first = doubles(nout * d), *total = doubles(nout * d);
	emulate_sensitivity_multi(emu, pca_space, lo, hi, e0, var, first, total);
	for (size_t t = 0; t < nout; t++)
		for (size_t j = 0, p = 0; j < d; j++)
			for (size_t k2 = j + 1; k2 < d; k2++, p++) inter_out[t * w + p] = vpair_out[t * w + p] - first[t * d + j] - first[t * d + k2];
	free(dev); free(cv); free(e0); free(var); free(first); free(total);
}

/* The posterior expectations E*[V_jk] and E*[V_jk - V_j - V_k] of every output (libemu.h): the plug-in half from
 * emulate_sensitivity_pairs_multi, cross terms and all; the S terms of the components through the SQUARED rule, as in
 * emulate_sensitivity_uncertainty_multi. */
void emulate_sensitivity_pairs_uncertainty_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, double *evpair_out,
                                                 double *einter_out)
{
	const size_t nr = (size_t)emu->nr, d = (size_t)emu->nparams, np = d * (d ? d - 1 : 0) / 2, w = 2 + 2 * d + np;
	const size_t nout = pca_space ? nr : (size_t)emu->nt;
	double *sc = doubles(nr * w), *so = doubles(nout * w);
	emulate_sensitivity_pairs_multi(emu, pca_space, lo, hi, evpair_out, einter_out);
	for (size_t c = 0; c < nr; c++) {
		emulate_sensitivity_post(emu->emu_struct_array[c], lo, hi, sc + c * w);
		emulate_sensitivity_pairs_post(emu->emu_struct_array[c], lo, hi, sc + c * w + 2 + 2 * d);
	}
	deliver(emu, pca_space, 1, 0, 1, w, sc, so);
	for (size_t t = 0; t < nout; t++) {
		const double *s = so + t * w, *sp = s + 2 + 2 * d;
		for (size_t j = 0, p = 0; j < d; j++)
			for (size_t k = j + 1; k < d; k++, p++) {
				evpair_out[t * np + p] += sp[p] - s[0];
				einter_out[t * np + p] += sp[p] - s[2 + j] - s[2 + k] + s[0];
			}
	}
	free(sc); free(so);
}

/* the two-way surface of every output on the grid gj x gk: joint_out and inter_out (may be NULL) are (ngrid x ngrid) x (nr or nt),
 * element ((a * ngrid + b) * nout + t); a conditional mean is linear in the components -- the mean half of the rule, the
 * training mean added to joint and to e0_out; the interaction effect has none */
void emulate_interaction_surface_multi(multi_emulator *emu, int pca_space, const double *lo, const double *hi, int j, int k, int ngrid,
                                       const double *gj, const double *gk, double *e0_out, double *joint_out, double *inter_out)
{
	const size_t nr = (size_t)emu->nr, g = (size_t)(ngrid > 0 ? ngrid : 0), np = g * g;
	double *jp = doubles(np * nr), *ip = doubles(np * nr), *jc = doubles(np ? np : 1), *ic = doubles(np ? np : 1), *ep = doubles(nr);
	for (size_t c = 0; c < nr; c++) {
		emulate_interaction_surface(emu->emu_struct_array[c], lo, hi, j, k, ngrid, gj, gk, &ep[c], jc, ic);
		place_component(jp, jc, np, nr, c, 1);
		place_component(ip, ic, np, nr, c, 1);
	}
	deliver(emu, pca_space, 0, 1, np, 1, jp, joint_out);
	if (inter_out) deliver(emu, pca_space, 0, 0, np, 1, ip, inter_out);
	deliver(emu, pca_space, 0, 1, 1, 1, ep, e0_out);
	free(jp); free(ip); free(jc); free(ic); free(ep);
}

static void one_point(multi_emulator *emu, gsl_vector *the_point, gsl_vector *the_mean, gsl_vector *the_variance, int pca_space)
{
	const int n = pca_space ? emu->nr : emu->nt;
	double *q = (double *)malloc(sizeof(double) * the_point->size);
	double *mo = (double *)malloc(sizeof(double) * (size_t)n), *vo = (double *)malloc(sizeof(double) * (size_t)n);
	for (size_t i = 0; i < the_point->size; i++) q[i] = gsl_vector_get(the_point, i);
	gsl_matrix view = gpemu_matrix_view(q, 1, the_point->size);
	emulate_points_multi(emu, &view, pca_space, mo, vo);
	for (int i = 0; i < n; i++) { gsl_vector_set(the_mean, i, mo[i]); gsl_vector_set(the_variance, i, vo[i]); }
	free(q); free(mo); free(vo);
}

/* multivar_support.c:78-86 */
void emulate_point_multi_pca(multi_emulator *emu, gsl_vector *the_point, gsl_vector *the_mean, gsl_vector *the_variance)
{
	one_point(emu, the_point, the_mean, the_variance, 1);
}

/* multivar_support.c:103-157 */
void emulate_point_multi(multi_emulator *emu, gsl_vector *the_point, gsl_vector *the_mean, gsl_vector *the_variance)
{
	one_point(emu, the_point, the_mean, the_variance, 0);
}
