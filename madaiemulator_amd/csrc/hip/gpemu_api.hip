// gpemu_api.hip -- C-ABI entry points (include/gpemu.h) and host-side
// orchestration of the gfx950 kernels: recursive tall-matrix Cholesky with the
// right-hand sides (and optionally the identity) riding along as extra rows,
// likelihood assembly, prediction set-up and the batched prediction sweep.
#include "gpemu_internal.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <climits>
#include <algorithm>

using namespace gpemu;

#define HIPCHK(ctx, call)                                                                       \
	do {                                                                                        \
		hipError_t e__ = (call);                                                                \
		if (e__ != hipSuccess) {                                                                \
			char buf__[512];                                                                    \
			snprintf(buf__, sizeof buf__, "%s:%d: %s -> %s", __FILE__, __LINE__, #call,         \
			         hipGetErrorString(e__));                                                   \
			(ctx)->err = buf__;                                                                 \
			return GPEMU_ERR_HIP;                                                               \
		}                                                                                       \
	} while (0)

constexpr int INFO_NONE = 0x7f7f7f7f;   // "no failed pivot": what hipMemsetAsync(.., 0x7f, ..) leaves in *info
static int pivot_info(int word) { return (word >= INFO_NONE) ? 0 : word; }   // 1-based index of the first failed pivot, 0: none

static int fail(gpemu_ctx *ctx, int code, const char *msg)
{
	if (ctx) ctx->err = msg;
	return code;
}

// the prediction state and the explicit inverse no longer belong to what the workspace, the model or the mode now say
// (nor does a resident joint factor, gpemu_predict_joint_factor: its buffers stay, its content is no longer offered)
static void invalidate_prediction(gpemu_ctx *ctx) { ctx->pred_ready = false; ctx->cinv_ready = false; ctx->linvT_ready = false; ctx->joint_M = 0; }

// ---------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------
static inline bool prof_on(gpemu_ctx *ctx, int cls) { return ctx->prof.cls == cls; }

static void prof_mark(gpemu_ctx *ctx)
{
	hipEvent_t e;
	hipEventCreate(&e);
	hipEventRecord(e, ctx->stream);
	ctx->prof.ev.push_back(e);
}

struct ProfScope {
	gpemu_ctx *ctx;
	bool on;
	ProfScope(gpemu_ctx *c, int cls, double flops, double bytes) : ctx(c), on(prof_on(c, cls))
	{
		if (on) {
			prof_mark(ctx);
			ctx->prof.flops += flops;
			ctx->prof.bytes += bytes;
			ctx->prof.n++;
		}
	}
	~ProfScope() { if (on) prof_mark(ctx); }
};

// GPEMU_TRACE: next {start,end} slot of the per-launch device timestamps (nullptr when tracing is off / full)
static unsigned long long *trace_slot(gpemu_ctx *ctx, const char *fmt, int a = 0, int b = 0, int c = 0)
{
	if (!ctx->dTrace || ctx->trace_next >= ctx->trace_cap) return nullptr;
	char buf[96];
	snprintf(buf, sizeof buf, fmt, a, b, c);
	ctx->trace_tag.push_back(buf);
	return ctx->dTrace + 8 * (size_t)ctx->trace_next++;
}

// GPEMU_TRACE: zeroed device slots for the launches that follow (nothing when tracing is off)
static hipError_t trace_clear(gpemu_ctx *ctx) { return ctx->dTrace ? hipMemsetAsync(ctx->dTrace, 0, (size_t)ctx->trace_cap * 64, ctx->stream) : hipSuccess; }

// algorithmic flops of one GEMM call: 2 * (k-range) summed over the output elements the call owns
// (lower trapezoid for tri; rows of an upper-triangular A start at k = row - kstart_off; rows of a
// lower-triangular B end at k = col - kend_off)
static double gemm_flops(const GemmArgs &a)
{
	double fl = 0.0;
	if (a.kend_mode) {
		for (int j = 0; j < a.n; j++) {
			int ke = std::min(a.k1, j + 1 - a.kend_off);
			if (ke > a.k0) fl += 2.0 * a.m * (double)(ke - a.k0);
		}
		return fl;
	}
	for (int i = 0; i < a.m; i++) {
		const int ncols = a.tri ? std::max(0, std::min(a.n, i + a.diag_off + 1)) : a.n;
		int kb = a.k0;
		if (a.kstart_mode) kb = std::max(kb, i - a.kstart_off);
		if (a.k1 > kb) fl += 2.0 * ncols * (double)(a.k1 - kb);
	}
	return fl;
}

// every schedule switch a GEMM call carries, in one list: gemm() applies it, and so does whoever asks about a call first or launches directly
static void apply_sched(const Sched &sc, GemmArgs &a)
{
	a.big_tiles = sc.gemm_big_tiles;
	a.table_sb = sc.gemm_table;
	a.keep_idle_waves = sc.idle_waves ? 0 : 1;
	a.stagger_ticks = sc.stagger_us * 100;
	a.row_table = sc.corner_row_table;
	a.no_neg_modifier = sc.neg_modifier ? 0 : 1;
}

static hipError_t gemm(gpemu_ctx *ctx, const GemmArgs &a_in)
{
	GemmArgs a = a_in;
	apply_sched(ctx->sched, a);
	a.trace = trace_slot(ctx, "gemm m=%d n=%d k=%d", a.m, a.n, a.k1 - a.k0);
	// GPEMU_PROF_GEMM: every GEMM launch; GPEMU_PROF_GEMM_BIG: only the launches that run the 128x128 8-wave kernel
	// (gemm_nt_kernel<128,128,4,4,2,0>, the dominant kernel of a batched factorisation); GPEMU_PROF_GEMM_K512: only
	// those with a contraction length of 512 or more (the compute-bound updates)
	const int cls = (prof_on(ctx, GPEMU_PROF_GEMM_BIG) && gemm_uses_big_tiles(a)) ? GPEMU_PROF_GEMM_BIG :
	                (prof_on(ctx, GPEMU_PROF_GEMM_K512) && a.k1 - a.k0 >= 512) ? GPEMU_PROF_GEMM_K512 : GPEMU_PROF_GEMM;
	const double fl = prof_on(ctx, cls) ? gemm_flops(a) * (a.nbatch > 1 ? a.nbatch : 1) : 0.0;
	ProfScope ps(ctx, cls, fl, 0.0);
	if (ps.on) {
		char buf[96];
		snprintf(buf, sizeof buf, "gemm m=%d n=%d k=%d tri=%d flops=%.4g", a.m, a.n, a.k1 - a.k0, a.tri, fl);
		ctx->prof.tag.push_back(buf);
	}
	return launch_gemm(ctx->stream, a);
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" const char *gpemu_version(void) { return "gpemu-mi355x 0.3 (gfx950, fp64 MFMA)"; }

extern "C" int gpemu_device_memory(int device, size_t *free_bytes, size_t *total_bytes)
{
	int n = 0, cur = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GPEMU_ERR_NO_DEVICE;
	if (device < 0 || device >= n) return GPEMU_ERR_ARG;
	size_t fr = 0, tot = 0;
	(void)hipGetDevice(&cur);
	const bool ok = hipSetDevice(device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess;
	if (!ok) (void)hipGetLastError();
	(void)hipSetDevice(cur);                   // the caller's current device, on the error path too
	if (!ok) return GPEMU_ERR_HIP;
	if (free_bytes) *free_bytes = fr;
	if (total_bytes) *total_bytes = tot;
	return GPEMU_OK;
}

extern "C" int gpemu_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// the schedule switches of a new context (gpemu::Sched): a variable that is absent or out of range gives the default
static Sched read_environment()
{
	auto geti = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
	Sched sc;
	int v = geti("GPEMU_GEMM_BIG_TILES", 1024);
	sc.gemm_big_tiles = v > 0 ? v : 1024;
	v = geti("GPEMU_GEMM_TABLE", 8);
	sc.gemm_table = v >= 0 && v <= 64 ? v : 8;
	sc.fill_gram = geti("GPEMU_FILL_GRAM", 1) != 0;
	sc.kvec_gram = geti("GPEMU_KVEC_GRAM", 1) != 0;
	sc.gemv_point = geti("GPEMU_GEMV_POINT", 1) != 0;
	sc.idle_waves = geti("GPEMU_IDLE_WAVES", 1) != 0;
	sc.neg_modifier = geti("GPEMU_NEG_MODIFIER", 1) != 0;
	sc.grad_gram = geti("GPEMU_GRAD_GRAM", 1) != 0;
	sc.stagger_us = std::max(0, std::min(1000, geti("GPEMU_STAGGER_US", 20)));
	sc.factor_ahead = geti("GPEMU_FACTOR_AHEAD", 1) != 0;
	sc.diag_inv_ahead = geti("GPEMU_DIAG_INV_AHEAD", 1) != 0;
	sc.leaf_pair = geti("GPEMU_LEAF_PAIR", 1) != 0;
	sc.corner_row_table = geti("GPEMU_CORNER_ROW_TABLE", 1) != 0;
	v = geti("GPEMU_LEAF_STAGED", -1);
	sc.leaf_staged = v == 0 || v == 1 ? v : -1;
	v = geti("GPEMU_NB_TOP", 0);
	sc.nb_top = v >= LEAF ? (v / LEAF) * LEAF : 0;
	sc.split_rhs_rows = geti("GPEMU_SPLIT_RHS_ROWS", 1) != 0;
	sc.rhs_ride = geti("GPEMU_RHS_RIDE", 1) != 0;
	v = geti("GPEMU_PANEL_ROWS", 1);
	sc.panel_rows = v >= 0 && v <= 2 ? v : 1;
	v = geti("GPEMU_PANEL_SPLIT", 1);
	sc.panel_split = v >= 0 && v <= (1 << 16) ? v : 1;
	v = geti("GPEMU_TARGET_PANEL", 2048);
	sc.target_panel = v >= 64 && v <= (1 << 16) && v % 64 == 0 ? v : 2048;
	return sc;
}

extern "C" int gpemu_ctx_create(gpemu_ctx **out, int device)
{
	if (!out) return GPEMU_ERR_ARG;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GPEMU_ERR_NO_DEVICE;
	if (device < 0 || device >= n) return GPEMU_ERR_ARG;
	if (hipSetDevice(device) != hipSuccess) return GPEMU_ERR_HIP;
	gpemu_ctx *ctx = new gpemu_ctx();
	ctx->sched = read_environment();
	ctx->device = device;
	ctx->res_len = 64 * 64 + 8;
	// the per-matrix result slots (three device and three pinned allocations: milliseconds) are made by the first
	// factorisation (ensure_batch_slots): a context that only ever answers queries -- a component of a multi-output emulator
	// set up by gpemu_predict_setup_batch -- never needs them
	int least = 0, greatest = 0;
	if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = 0; greatest = 0; }
	bool ok = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest) == hipSuccess;
	for (int i = 0; ok && i < gpemu_ctx::RES_RING; i++)
		ok = hipEventCreateWithFlags(&ctx->ring[i].ev, hipEventDisableTiming) == hipSuccess;
	const char *tr = getenv("GPEMU_TRACE");
	if (ok && tr && atoi(tr) > 0) {                 // in-kernel timestamps: 4096 launch slots of 8 x u64
		ctx->trace_cap = 4096;
		if (ctx->dTrace.grow((size_t)ctx->trace_cap * 8) != hipSuccess) ctx->trace_cap = 0;
	}
	const char *ng = getenv("GPEMU_NO_GRAPH");
	if (ng && ng[0] == '1') ctx->use_graph = false;
	{
		const char *eg = getenv("GPEMU_EXACT_GRAD"), *mf = getenv("GPEMU_MATERN_FIXED");
		if (eg && atoi(eg) > 0) ctx->mode |= GPEMU_MODE_EXACT_GRAD;
		if (mf && atoi(mf) > 0) ctx->mode |= GPEMU_MODE_MATERN_LOG;
	}
	if (!ok) {
		(void)hipGetLastError();
		gpemu_ctx_destroy(ctx);
		return GPEMU_ERR_HIP;
	}
	*out = ctx;
	return GPEMU_OK;
}

static void free_graphs(gpemu_ctx *ctx)
{
	for (auto &kv : ctx->graphs) hipGraphExecDestroy(kv.second);
	ctx->graphs.clear();
	ctx->warm.clear();
}

// The one way a buffer of a context grows.  Nothing but a compare when it is large enough; otherwise enqueued work that may
// still use the old allocation is waited for, then release and allocate (contents are not kept).  graphed: the cached launch
// graphs hold the buffer's address -- dT and dInfo, which is all potrf_rec touches that can move -- and go when it moves.
// oom: the message of a failed allocation (the error is then cleared); none: the runtime's own, like any failed call.
template <class B>
static int grow(gpemu_ctx *ctx, B &buf, size_t n, bool graphed = false, const char *oom = nullptr)
{
	if (buf.size() >= n) return GPEMU_OK;
	if (graphed) free_graphs(ctx);
	if (buf) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	const hipError_t e = buf.grow(n);
	if (e != hipSuccess && oom) {
		(void)hipGetLastError();
		return fail(ctx, GPEMU_ERR_HIP, oom);
	}
	HIPCHK(ctx, e);
	return GPEMU_OK;
}

// the target set of gpemu_design_target_* and everything those entries keep (the caller has waited for the stream)
static void free_targets(gpemu_ctx *ctx)
{
	for (auto *b : {&ctx->dTgtX, &ctx->dTgtW, &ctx->dTgtU, &ctx->dTgtR, &ctx->dTgtQr, &ctx->dTgtVar, &ctx->dTgtSum, &ctx->dTgtCR, &ctx->dTgtPanel,
	                &ctx->dTgtPart, &ctx->dTgtScr, &ctx->dTgtIO})
		b->reset();
	ctx->tgt_S = ctx->tgt_mb = 0;
	ctx->tgt_serial = 0;
}

// everything sized by the model (the per-matrix result slots, the symmetric-matrix cache and the upload ring stay)
static void free_model(gpemu_ctx *ctx)
{
	free_graphs(ctx);
	for (auto *b : {&ctx->dX, &ctx->dXg, &ctx->dMid, &ctx->dY, &ctx->dRrows, &ctx->dT, &ctx->dGramPart, &ctx->dLinvAug, &ctx->dBetaQ,
	                &ctx->dKq, &ctx->dV, &ctx->dXq, &ctx->dMean, &ctx->dS, &ctx->dGradPart, &ctx->dAlpha,
	                &ctx->dLooPart, &ctx->dLoo, &ctx->dMeanPart, &ctx->dMGradPart, &ctx->dMGrad, &ctx->dLinvAugT, &ctx->dVGradPart, &ctx->dCovR,
	                &ctx->dCov, &ctx->dJoint, &ctx->dJointMean, &ctx->dJointPart, &ctx->dJointZ, &ctx->dJointIO})
		b->reset();
	ctx->dJointInfo.reset();
	for (auto *b : {&ctx->dLgoZ, &ctx->dLgoT, &ctx->dLgoPart, &ctx->dLgoOut}) b->reset();
	for (auto *b : {&ctx->dLgoTab, &ctx->dLgoInfo, &ctx->dLgoInfoOut}) b->reset();
	ctx->hLgoTab.reset();
	for (auto *b : {&ctx->dSensPrep, &ctx->dSensCst, &ctx->dSensPart, &ctx->dSensOut, &ctx->dSensGrid, &ctx->dSensP, &ctx->dSensG,
	                &ctx->dSensPostPart, &ctx->dSensPex2, &ctx->dSensPairPart, &ctx->dSensPairOut})
		b->reset();
	ctx->sens_post_N = 0;
	for (auto *b : {&ctx->dDesignKH, &ctx->dDesignHm, &ctx->dDesignPrepQ, &ctx->dDesignA, &ctx->dDesignT, &ctx->dDesignR, &ctx->dDesignB,
	                &ctx->dDesignPart, &ctx->dDesignOut})
		b->reset();
	ctx->design_serial = 0;
	ctx->design_mb = 0;
	for (auto *b : {&ctx->dBatchW, &ctx->dBatchLam, &ctx->dBatchMu, &ctx->dBatchE, &ctx->dBatchSv, &ctx->dBatchDots, &ctx->dBatchSt, &ctx->dBatchTab,
	                &ctx->dBatchIO})
		b->reset();
	ctx->batch_mb = ctx->batch_nb = 0;
	free_targets(ctx);
	ctx->hStage.reset();
	ctx->hLoo.reset();
	ctx->hMGrad.reset();
	invalidate_prediction(ctx);
	ctx->pred_pending = {};
	ctx->S_dim = 0;
}

gpemu_ctx::~gpemu_ctx()
{
	hipSetDevice(device);
	if (stream) hipStreamSynchronize(stream);
	free_model(this);
	for (auto e : prof.ev) hipEventDestroy(e);
	for (auto e : pring.ev) if (e) hipEventDestroy(e);
	if (lgo_ev) hipEventDestroy(lgo_ev);
	if (sens_ev) hipEventDestroy(sens_ev);
	if (sens_ev2) hipEventDestroy(sens_ev2);
	for (auto &s : ring) if (s.ev) hipEventDestroy(s.ev);
	if (stream) hipStreamDestroy(stream);
}

extern "C" void gpemu_ctx_destroy(gpemu_ctx *ctx) { delete ctx; }

extern "C" int gpemu_set_mode(gpemu_ctx *ctx, int flags)
{
	if (!ctx || (flags & ~(GPEMU_MODE_EXACT_GRAD | GPEMU_MODE_MATERN_LOG))) return GPEMU_ERR_ARG;
	if (flags != ctx->mode) invalidate_prediction(ctx);   // the kernel's meaning may have changed
	ctx->mode = flags;
	return GPEMU_OK;
}
extern "C" int gpemu_get_mode(const gpemu_ctx *ctx) { return ctx ? ctx->mode : 0; }

extern "C" const char *gpemu_last_error(const gpemu_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }
extern "C" int gpemu_ctx_device(const gpemu_ctx *ctx) { return ctx ? ctx->device : -1; }

extern "C" int gpemu_sync(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

extern "C" int gpemu_dev_alloc(gpemu_ctx *ctx, size_t bytes, void **dptr)
{
	if (!ctx || !dptr) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, DeviceMem::alloc(dptr, bytes));
	return GPEMU_OK;
}
extern "C" int gpemu_dev_free(gpemu_ctx *ctx, void *dptr)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, DeviceMem::release(dptr));
	return GPEMU_OK;
}
extern "C" int gpemu_dev_upload(gpemu_ctx *ctx, void *dst, const void *src, size_t bytes)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}
extern "C" int gpemu_dev_download(gpemu_ctx *ctx, void *dst, const void *src, size_t bytes)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
// workspace for nb tall matrices of rows_each rows, packed one after the other (stride rows_each * Np)
static int ensure_T(gpemu_ctx *ctx, size_t rows_each, int nb = 1)
{
	ctx->nb = nb;
	ctx->T_stride = rows_each * (size_t)ctx->Np;
	return grow(ctx, ctx->dT, ctx->T_stride * (size_t)nb, true, "out of device memory for the factorisation workspace (smaller batch?)");
}

// per-matrix result slots (info word, Gram partials, Gram + log det, pinned mirrors) for a batch of nb
static int ensure_batch_slots(gpemu_ctx *ctx, int nb)
{
	if (nb > ctx->batch_cap()) {
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		ctx->res_seq = 0;                      // results still in the old ring are gone with it
		ctx->dInfo.reset();                    // (the capacity is zero until all of them are there again)
		const size_t n = (size_t)nb, rn = (size_t)gpemu_ctx::RES_RING * n;
		int rc = grow(ctx, ctx->dRes, n * ctx->res_len);
		if (!rc) rc = grow(ctx, ctx->hResRing, rn * ctx->res_len);
		if (!rc) rc = grow(ctx, ctx->hInfoRing, rn);
		if (!rc) rc = grow(ctx, ctx->dGradSum, n * gpemu_ctx::GRAD_NP_MAX);
		if (!rc) rc = grow(ctx, ctx->hGradRing, rn * gpemu_ctx::GRAD_NP_MAX);
		if (!rc) rc = grow(ctx, ctx->dInfo, n, true);
		if (rc) return rc;
		for (size_t i = 0; i < (size_t)gpemu_ctx::RES_RING; i++) {
			ResSlot &s = ctx->ring[i];
			s.nb = 0;
			s.res = ctx->hResRing + i * n * ctx->res_len;
			s.info = ctx->hInfoRing + i * n;
			s.grad = ctx->hGradRing + i * n * gpemu_ctx::GRAD_NP_MAX;
		}
	}
	return grow(ctx, ctx->dGramPart, (size_t)ctx->batch_cap() * (ctx->Np / 64) * ctx->Rp * ctx->Rp);
}

extern "C" int gpemu_set_model(gpemu_ctx *ctx, int kind, int order, int N, int d, const double *X, const double *y)
{
	if (!ctx || !X || !y) return GPEMU_ERR_ARG;
	if (kind < GPEMU_POWEREXP || kind > GPEMU_MATERN52) return fail(ctx, GPEMU_ERR_ARG, "bad cov_fn_index");
	if (order < 0 || order > 3) return fail(ctx, GPEMU_ERR_ARG, "regression_order must be 0..3");
	if (N < 1 || d < 1 || d > GPEMU_MAX_PARAMS) return fail(ctx, GPEMU_ERR_ARG, "bad N or nparams");
	const int nreg = 1 + order * d;
	if (nreg + 1 > 64) return fail(ctx, GPEMU_ERR_ARG, "1 + nregression_fns must be <= 64");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	free_model(ctx);
	std::fill(ctx->sens_kind, ctx->sens_kind + GPEMU_MAX_PARAMS, GPEMU_MEASURE_UNIFORM);   // d may change: the measure starts over
	ctx->res_seq = 0;                       // batches of the previous model can no longer be collected (their sizes are gone)
	ctx->kind = kind; ctx->order = order; ctx->N = N; ctx->d = d; ctx->nreg = nreg; ctx->nrhs = nreg + 1;
	ctx->Np = round_up(N, LEAF);
	ctx->Rp = 64;
	ctx->hX.assign(X, X + (size_t)N * d);
	ctx->hY.assign(y, y + N);
	HIPCHK(ctx, ctx->dX.grow((size_t)N * d));
	HIPCHK(ctx, ctx->dY.grow((size_t)N));
	HIPCHK(ctx, ctx->dRrows.grow((size_t)ctx->Rp * ctx->Np));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dX, ctx->hX.data(), (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dY, ctx->hY.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	{
		// the design centred per dimension (operands of the Gram-form fill) and the half ranges that bound its error
		std::vector<double> lo(d, HUGE_VAL), hi(d, -HUGE_VAL), xg((size_t)N * d);
		bool finite = true;
		for (int i = 0; i < N; i++)
			for (int k = 0; k < d; k++) {
				const double v = X[(size_t)i * d + k];
				if (!(fabs(v) <= 1e300)) finite = false;
				if (v < lo[k]) lo[k] = v;
				if (v > hi[k]) hi[k] = v;
			}
		ctx->xhalf.assign(d, HUGE_VAL);
		if (finite) {
			for (int k = 0; k < d; k++) ctx->xhalf[k] = 0.5 * (hi[k] - lo[k]);
			for (int i = 0; i < N; i++)
				for (int k = 0; k < d; k++) xg[(size_t)i * d + k] = X[(size_t)i * d + k] - 0.5 * (hi[k] + lo[k]);
			HIPCHK(ctx, ctx->dXg.grow((size_t)N * d));
			// (on the context's own stream, never the legacy stream: a plain hipMemcpy fails with "operation would make the
			// legacy stream depend on a capturing blocking stream" while ANOTHER host thread records its launch graph)
			HIPCHK(ctx, hipMemcpyAsync(ctx->dXg, xg.data(), (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
			std::vector<double> mid(d);
			for (int k = 0; k < d; k++) mid[k] = 0.5 * (hi[k] + lo[k]);
			HIPCHK(ctx, ctx->dMid.grow((size_t)d));
			HIPCHK(ctx, hipMemcpyAsync(ctx->dMid, mid.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
			HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		}
	}
	HIPCHK(ctx, launch_build_rrows(ctx->stream, ctx->dRrows, ctx->Np, ctx->Rp, ctx->dX, ctx->dY, N, d, order));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	// (the factorisation workspace is made by the first factorisation, stage_matrices: a context whose prediction state comes
	// from gpemu_predict_setup_batch never factors anything itself)
	return GPEMU_OK;
}

extern "C" int gpemu_set_training(gpemu_ctx *ctx, const double *y)
{
	if (!ctx || !y || !ctx->dX) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->hY.assign(y, y + ctx->N);
	HIPCHK(ctx, hipMemcpyAsync(ctx->dY, ctx->hY.data(), (size_t)ctx->N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, launch_build_rrows(ctx->stream, ctx->dRrows, ctx->Np, ctx->Rp, ctx->dX, ctx->dY, ctx->N, ctx->d, ctx->order));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	invalidate_prediction(ctx);
	return GPEMU_OK;
}

static int nthetas_for(const gpemu_ctx *ctx) { return ctx->kind == GPEMU_POWEREXP ? ctx->d + 2 : 3; }

// theta layout: modelstruct.c:300-308.  pow-exp exponentiates everything
// (emulator.c:115-123); the Matern kernels take amp and nugget raw (:355-357).
// norm2_out (optional): the admission rule's sum_k (w_k halfrange_k)^2, NaN for a design without a centred copy
static int make_cov_params(gpemu_ctx *ctx, const double *thetas, int nthetas, CovParams *p, double *norm2_out = nullptr)
{
	if (norm2_out) *norm2_out = NAN;
	if (!thetas) return fail(ctx, GPEMU_ERR_ARG, "thetas is NULL");
	if (nthetas < nthetas_for(ctx)) return fail(ctx, GPEMU_ERR_ARG, "nthetas too small for this covariance function");
	memset(p, 0, sizeof *p);
	p->kind = ctx->kind;
	p->d = ctx->d;
	if (ctx->kind == GPEMU_POWEREXP) {
		p->amp = exp(thetas[0]);
		p->nug = exp(thetas[1]);
		p->eps = 0.0000000001;
		double wmax = 0.0;
		for (int k = 0; k < ctx->d; k++) {
			double r = exp(thetas[k + 2]);
			p->w[k] = sqrt(0.5) / r;
			if (p->w[k] > wmax) wmax = p->w[k];
		}
		p->cand = 2.0 * ctx->d * (p->eps * wmax) * (p->eps * wmax) + 1e-300;
	} else {
		// literal (emulator.c:355-356, 448-449): amplitude and nugget are used as they come.  GPEMU_MODE_MATERN_LOG
		// (SURVEY App. C2 "fixed mode"): both on the log scale like the pow-exp kernel's, so that evalFnMulti's
		// theta[0] = 0 (maxmultimin.c:311) means amplitude 1 and the model can be trained.
		const bool logscale = (ctx->mode & GPEMU_MODE_MATERN_LOG) != 0;
		p->amp = logscale ? exp(thetas[0]) : thetas[0];
		p->nug = logscale ? exp(thetas[1]) : thetas[1];
		p->eps = 0.0000000000000001;
		p->w[0] = 1.0 / exp(thetas[2]);
		p->cand = 2.0 * ctx->d * (p->eps * p->w[0]) * (p->eps * p->w[0]) + 1e-300;
	}
	// Gram form of the training fill (kernels_cov.hip): only while the centred, scaled design stays small -- the
	// cancellation error of |x'|^2 + |y'|^2 - 2 x'.y' is a few ulp of 2 * norm2
	p->gram = 0; p->cand_g = 0.0; p->cand_w = p->cand;
	if (ctx->dXg && (int)ctx->xhalf.size() == ctx->d) {
		double norm2 = 0.0;
		for (int k = 0; k < ctx->d; k++) {
			const double t = ctx->xhalf[k] * p->w[ctx->kind == GPEMU_POWEREXP ? k : 0];
			norm2 += t * t;
		}
		if (norm2_out) *norm2_out = norm2;
		// the candidates of the nugget rule in a Gram-form distance: below the difference form's bound plus the form's own
		// cancellation error (a few ulp of |x'|^2 + |y'|^2 <= 2 norm2, 64 ulp allowed), whatever the length scales
		p->cand_w = p->cand + 64.0 * 2.220446049250313e-16 * (2.0 * norm2 + 1.0);
		if (ctx->sched.fill_gram && norm2 <= 16.0) {
			p->gram = 1;
			p->cand_g = p->cand_w;
		}
	}
	return GPEMU_OK;
}

// nb theta vectors, nthetas apart -> their CovParams
static int make_cov_params_batch(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas, std::vector<CovParams> *ps)
{
	ps->resize((size_t)nb);
	int rc = GPEMU_OK;
	for (int b = 0; !rc && b < nb; b++) rc = make_cov_params(ctx, thetas ? thetas + (size_t)b * nthetas : nullptr, nthetas, &(*ps)[b]);
	return rc;
}

// ---------------------------------------------------------------------------
// recursive tall Cholesky
//   T rows [0,Np)            : C (lower), identity padded
//   T rows [Np,Np+Rp)        : right-hand sides as rows (y, H columns) -> Z^T = (L^-1 [y|H])^T
//   T rows [Np+Rp,Np+Rp+Np)  : identity -> U = L^-T (only with inv)
// potrf_rec(c0,n) factors the column panel [c0,c0+n) for every row below it.
// The matrices come as a view (Tall); stream, schedule switches, profiling and trace are the context's.
// ---------------------------------------------------------------------------
// (the context's own workspace as it stands: after staging, which sets nb and the stride, and never kept across calls)
static Tall tall_of(gpemu_ctx *ctx) { return Tall{ctx->dT, ctx->dInfo, ctx->Np, ctx->Rp, ctx->nb, (long)ctx->T_stride, ctx->nrhs}; }

// *fa_done: set when the update ran with the factor-ahead tile, i.e. the 64x64 diagonal block at c0+k is already
// factored when the update has finished and the next leaf must not factor it again
// row_cut > 0 (without inverse rows): the update stops at that row -- the rows from there on are panel_rows_kernel's
// ride: 1 / 0 = riders on / off for this call, -1 = the context's GPEMU_RHS_RIDE (what production passes)
static hipError_t trailing_update(gpemu_ctx *ctx, const Tall &t, int c0, int k, int ncols, int inv, bool *fa_done, int row_cut = 0,
                                  int ride = -1)
{
	// C[rows >= r0, cols r0 .. r0+ncols) -= P P^T with P = the factored panel columns [c0, c0+k) and r0 = c0 + k
	const long ld = t.Np;
	const int r0 = c0 + k;
	const int row_end = row_cut > 0 ? row_cut : t.Np + t.Rp + (inv ? c0 + k : 0);   // identity rows < c0+k have fill-in in the panel
	GemmArgs g{};
	g.C = t.T + (long)r0 * ld + r0;
	g.A = t.T + (long)r0 * ld + c0;
	g.B = g.A;
	g.ldc = g.lda = g.ldb = ld;
	g.m = row_end - r0;
	g.n = ncols;
	g.k0 = 0; g.k1 = k;
	g.alpha = -1.0; g.beta = 1;
	g.tri = 1; g.diag_off = 0;
	g.nbatch = t.nb; g.bsC = g.bsA = g.bsB = t.stride;
	apply_sched(ctx->sched, g);                                   // (gemm() does too: here for the tile-shape questions below)
	g.fa = ctx->sched.factor_ahead ? 1 : 0;
	g.fa_c0 = r0;
	g.fa_info = t.info;
	*fa_done = g.fa && gemm_factor_ahead_ok(g);
	if (!*fa_done) g.fa = 0;
	const int c_rows = t.Np - r0;                                 // rows of the matrix proper under r0
	if (ctx->sched.split_rhs_rows && gemm_uses_big_tiles(g) && c_rows % GEMM_BM == 0 && c_rows >= ncols && g.m > c_rows) {
		// 128x128 tiles: the 64 right-hand-side rows between the matrix rows and the identity rows would shift every tile row
		// behind them by half a tile and leave the last one half empty (2-5 % of the tile slots of a big update: 48 of 1224
		// at the first update of a batch at N = 8192).  Three launches instead: the matrix rows (triangular part, full 128-row
		// tiles), the right-hand-side rows on 64x64 tiles, the identity rows (gradient / inverse only).  Same k-ordered chain
		// per element whatever the tile shape: the bits do not change.
		// Riders (GPEMU_RHS_RIDE): when at most 16 of the right-hand-side rows can be non-zero, the idle waves of the matrix
		// rows' diagonal tiles take them (gemm_nt_kernel, RIDE) and the second launch is dropped: it read the whole panel a
		// second time for 64 rows of which 48 and more are 0 - 0 b.  Rows 16 .. Rp-1 are then not touched: +0 before and after
		// for finite operands.  (A panel with Inf or NaN in it -- after a failed pivot -- made them NaN in the old launch and
		// leaves them +0 here; nothing reads them, the Gram and finish kernels take nrhs rows, and the info word reports the pivot.)
		GemmArgs a = g;
		a.m = c_rows;
		if ((ride < 0 ? ctx->sched.rhs_ride : ride) && t.rhs_live > 0 && t.rhs_live <= 16 && t.Rp >= 16 && ncols % GEMM_BM == 0) {
			a.ride_C = g.C + (long)c_rows * ld; a.ride_A = g.A + (long)c_rows * ld; a.ride_rows = 16;
			if (!gemm_ride_ok(a)) { a.ride_C = nullptr; a.ride_A = nullptr; a.ride_rows = 0; }
		}
		hipError_t e = gemm(ctx, a);
		if (e != hipSuccess) return e;
		if (!a.ride_rows) {
			GemmArgs b = g;
			b.C = g.C + (long)c_rows * ld; b.A = g.A + (long)c_rows * ld;
			b.m = t.Rp; b.tri = 0; b.force_cfg = 2;
			e = gemm(ctx, b);
			if (e != hipSuccess) return e;
		}
		const int i_rows = g.m - c_rows - t.Rp;
		if (i_rows > 0) {
			GemmArgs c = g;
			c.C = g.C + (long)(c_rows + t.Rp) * ld; c.A = g.A + (long)(c_rows + t.Rp) * ld;
			c.m = i_rows; c.tri = 0;
			e = gemm(ctx, c);
		}
		return e;
	}
	return gemm(ctx, g);
}

// diag_done: the 64x64 diagonal block at (c0,c0) is already factored (by the factor-ahead tile of the update before)
// defer_c0 >= 0: the leaf solve of this block also solves, in place, the 64 rows under the diagonal block at defer_c0 (the
// pair's first block, which leaf_pair_kernel leaves untouched there)
// panel_end: the end of the diagonal square of the outer panel this node lies in (0: this node is the outer panel)
// row_cut > 0 (without inverse rows): the node's launches stop at that row -- a 256-column group whose rows from there on
// go through panel_rows_kernel
static hipError_t potrf_rec(gpemu_ctx *ctx, const Tall &t, int c0, int n, int inv, bool diag_done = false, int defer_c0 = -1,
                            int panel_end = 0, int row_cut = 0)
{
	const long ld = t.Np;
	const int base_end = row_cut > 0 ? row_cut : t.Np + t.Rp;
	if (n <= LEAF) {
		const int row_end = base_end + (inv ? c0 + LEAF : 0);
		ProfScope ps(ctx, GPEMU_PROF_LEAF, 0.0, 0.0);
		unsigned long long *trf = trace_slot(ctx, "leaf_factor c0=%d", c0);
		unsigned long long *trs = trace_slot(ctx, "leaf_solve c0=%d m=%d", c0, row_end - (c0 + LEAF));
		return launch_leaf(ctx->stream, t.T, ld, c0, row_end - (c0 + LEAF), t.info, trf, trs, t.nb, t.stride, diag_done,
		                   ctx->sched.leaf_staged, ctx->sched.diag_inv_ahead != 0, defer_c0);
	}
	if (n == 2 * LEAF && ctx->sched.leaf_pair && ctx->sched.diag_inv_ahead) {
		// a 128-column pair: [factor the first diagonal block,] leaf_pair_kernel (solve of the first block + K=64 update with
		// its factor-ahead tile), then the second block's leaf solve with the deferred 64 rows of the first
		const int row_end = base_end + (inv ? c0 + LEAF : 0);
		const int m_below = row_end - (c0 + LEAF);
		ProfScope ps(ctx, GPEMU_PROF_LEAF, 0.0, 0.0);
		if (!diag_done) {
			unsigned long long *trf = trace_slot(ctx, "leaf_factor c0=%d", c0);
			hipError_t e = launch_leaf(ctx->stream, t.T, ld, c0, 0, t.info, trf, nullptr, t.nb, t.stride, false);
			if (e != hipSuccess) return e;
		}
		unsigned long long *trp = trace_slot(ctx, "leaf_pair c0=%d m=%d", c0, m_below);
		const bool fa = ctx->sched.factor_ahead != 0;
		hipError_t e = launch_leaf_pair(ctx->stream, t.T, ld, c0, m_below, t.info, trp, t.nb, t.stride, fa);
		if (e != hipSuccess) return e;
		return potrf_rec(ctx, t, c0 + LEAF, LEAF, inv, fa, c0, panel_end, row_cut);
	}
	// automatic outer panel width: a batch has enough tiles per launch to afford the longer panel chain of a wider
	// panel and gains from the larger K of its trailing updates and the fewer read-modify-write passes over the
	// trailing matrix (measured at 2x16, N=8192: 3.77 ms per evaluation at 512, 3.55 at 1024 with the first GEMM
	// epilogue; 3.329 at 1024, 3.302 at 2048, 3.314 at 4096 now; 2048 also wins at N = 4096, 12288, 16384)
	// With the inverse rows under the matrix (gradient, explicit inverse) 1024 is better again: 10.40 against 10.77 ms
	// per value+gradient evaluation in batches of 16.
	// Round 5, measured at N = 4096 (profiles/r05_n4096_schedule_switches.txt): with the inverse rows 512 beats 1024 there
	// (value+gradient batches of 16 / 64: +2 %), without them 1024 .. 4096 are within 0.5 % of each other.
	const int nb_top = ctx->sched.nb_top > 0 ? ctx->sched.nb_top : (t.nb >= 2 ? (inv ? (t.Np <= 4096 ? 512 : 1024) : 2048) : 512);
	if (n > nb_top) {
		// right-looking over panels of nb_top columns: the trailing update touches the whole remaining
		// matrix (thousands of tiles, K = panel width), which fills the chip far better than the few huge-K
		// tiles a pure recursion would produce at the top levels
		bool next_done = diag_done;
		for (int c = c0; c < c0 + n; c += nb_top) {
			const int nb = std::min(nb_top, c0 + n - c);
			hipError_t e = potrf_rec(ctx, t, c, nb, inv, next_done, -1, c + nb);
			next_done = false;
			if (e != hipSuccess) return e;
			const int rest = c0 + n - (c + nb);
			if (rest <= 0) continue;
			e = trailing_update(ctx, t, c, nb, rest, inv, &next_done);
			if (e != hipSuccess) return e;
		}
		return hipSuccess;
	}
	if (panel_end == 0) panel_end = c0 + n;
	if (n == 4 * LEAF && !inv && row_cut == 0 && ctx->sched.panel_rows && ctx->sched.leaf_pair && ctx->sched.diag_inv_ahead) {
		// a 256-column group: its five launches (pair, solve, K = 128 update, pair, solve) stop at r_split, and the rows from
		// there on -- operands of later updates only, the right-hand sides among them -- take the group's whole arithmetic in
		// one pass (panel_rows_kernel; same bits).  Every cut launch keeps arguments it accepts today: at least 64 rows under
		// the group for the last solve (with the cut at the end of the outer panel's square the panel's last group stays as
		// it is).  The cut 64 rows under the group, the most rows the one pass can take, measured best.
		// Automatic: lock-step batches whose launch fills the chip's resident workgroups once (two per CU); one matrix is
		// latency-bound and must not get a launch more per group.
		const int r_split = ctx->sched.panel_split > 0 ? c0 + 4 * LEAF + LEAF * ctx->sched.panel_split : panel_end;
		const int m_far = base_end - r_split;
		const bool big = ctx->sched.panel_rows == 2 || (t.nb >= 2 && (long)(m_far / LEAF) * t.nb >= 512);
		if (big && r_split >= c0 + 5 * LEAF && m_far >= LEAF && m_far % LEAF == 0) {
			hipError_t e = potrf_rec(ctx, t, c0, n, inv, diag_done, -1, panel_end, r_split);
			if (e != hipSuccess) return e;
			ProfScope ps(ctx, GPEMU_PROF_LEAF, 0.0, 0.0);
			unsigned long long *trp = trace_slot(ctx, "panel_rows cg=%d m=%d", c0, m_far);
			return launch_panel_rows(ctx->stream, t.T, ld, c0, r_split, m_far, trp, t.nb, t.stride);
		}
	}
	const int n1 = ((n / LEAF + 1) / 2) * LEAF;
	hipError_t e = potrf_rec(ctx, t, c0, n1, inv, diag_done, -1, panel_end, row_cut);
	if (e != hipSuccess) return e;
	bool right_done = false;
	e = trailing_update(ctx, t, c0, n1, n - n1, inv, &right_done, row_cut);
	if (e != hipSuccess) return e;
	return potrf_rec(ctx, t, c0 + n1, n - n1, inv, right_done, -1, panel_end, row_cut);
}

// the whole factorisation with plain launches (or under capture), its trace tags from slot 0
static hipError_t potrf_all(gpemu_ctx *ctx, const Tall &t, int inv)
{
	ctx->trace_next = 0; ctx->trace_tag.clear();
	return potrf_rec(ctx, t, 0, t.Np, inv);
}

static int run_potrf(gpemu_ctx *ctx, int inv)
{
	const Tall t = tall_of(ctx);
	const bool profiling = ctx->prof.cls == GPEMU_PROF_GEMM || ctx->prof.cls == GPEMU_PROF_LEAF || ctx->prof.cls == GPEMU_PROF_GEMM_BIG ||
	                       ctx->prof.cls == GPEMU_PROF_GEMM_K512;
	HIPCHK(ctx, trace_clear(ctx));
	double fl = (double)ctx->nb * ctx->Np * ctx->Np * ctx->Np / 3.0;
	ProfScope ps(ctx, GPEMU_PROF_POTRF, fl, 0.0);
	const gpemu_ctx::GraphKey key{ctx->Np, ctx->Rp, inv, ctx->nb};
	auto it = ctx->graphs.find(key);
	// plain launches: without graphs, under profiling, and for the first factorisation of a shape (host-side tables of the
	// GEMM tile order are built on first use and cannot be allocated under stream capture); the next call records the graph
	if (!ctx->use_graph || profiling || (it == ctx->graphs.end() && ctx->warm.insert(key).second)) {
		HIPCHK(ctx, potrf_all(ctx, t, inv));
		return GPEMU_OK;
	}
	if (it == ctx->graphs.end()) {
		hipGraph_t graph = nullptr;
		HIPCHK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
		hipError_t e = potrf_all(ctx, t, inv);
		hipError_t e2 = hipStreamEndCapture(ctx->stream, &graph);
		if (e != hipSuccess || e2 != hipSuccess) {
			if (graph) hipGraphDestroy(graph);
			ctx->err = "potrf graph capture failed";
			return GPEMU_ERR_HIP;
		}
		hipGraphExec_t exec = nullptr;
		HIPCHK(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
		hipGraphDestroy(graph);
		it = ctx->graphs.emplace(key, exec).first;
	}
	HIPCHK(ctx, hipGraphLaunch(it->second, ctx->stream));
	return GPEMU_OK;
}

// fill C(theta_b) into matrix b of T (lower tiles only), load the RHS rows, reset the info words
// rrows / rstride: right-hand-side rows of the batch when they are not the context's own (rstride != 0: matrix b takes
// rrows + b * rstride -- the components of a multi-output model, gpemu_predict_setup_batch)
static int stage_matrices(gpemu_ctx *ctx, const CovParams *ps, int nb, int inv, const double *rrows = nullptr, long rstride = 0)
{
	const int Np = ctx->Np, Rp = ctx->Rp;
	int rc = ensure_batch_slots(ctx, nb);
	if (rc) return rc;
	rc = ensure_T(ctx, (size_t)Np + Rp + (inv ? Np : 0), nb);
	if (rc) return rc;
	// one upload of the nb hyper-parameter sets, one launch for the nb fills and R-row copies.  The upload goes through a
	// pinned ring of four entries (a pageable source makes hipMemcpyAsync wait for the stream: enqueued batches of small
	// models then take 6 us per evaluation instead of 2); an entry is reused once its own copy has executed.
	ParamRing &pr = ctx->pring;
	if (!ctx->dParams) {                   // (allocated last: there means that the ring is complete)
		HIPCHK(ctx, pr.params.grow((size_t)ParamRing::RING * GPEMU_MAX_BATCH));
		HIPCHK(ctx, pr.gph.grow((size_t)ParamRing::RING * GPEMU_MAX_BATCH * GPEMU_MAX_PARAMS));
		for (auto &e : pr.ev) if (!e) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
		HIPCHK(ctx, ctx->dParams.grow((size_t)GPEMU_MAX_BATCH));
	}
	{
		pr.slot = pr.next++ % ParamRing::RING;
		HIPCHK(ctx, hipEventSynchronize(pr.ev[pr.slot]));             // (a never-recorded event is complete)
		CovParams *hp = pr.params + (size_t)pr.slot * GPEMU_MAX_BATCH;
		memcpy(hp, ps, (size_t)nb * sizeof(CovParams));
		HIPCHK(ctx, hipMemcpyAsync(ctx->dParams, hp, (size_t)nb * sizeof(CovParams), hipMemcpyHostToDevice, ctx->stream));
		HIPCHK(ctx, hipEventRecord(pr.ev[pr.slot], ctx->stream));
	}
	{
		const double nlow = 0.5 * (double)Np * Np * nb;
		ProfScope ps_(ctx, GPEMU_PROF_FILL, 0.0, 8.0 * nlow);
		bool all_gram = ctx->dXg != nullptr;
		for (int b = 0; b < nb; b++) all_gram = all_gram && ps[b].gram;
		HIPCHK(ctx, launch_cov_stage_batch(ctx->stream, ctx->dT, Np, (long)ctx->T_stride, nb, ctx->dX, ctx->N, Np, ctx->d,
		                                   ctx->dParams, FILL_LOWER | FILL_IDENT_PAD, rrows ? rrows : ctx->dRrows, Rp, ctx->dXg, all_gram,
		                                   ctx->kind, rrows ? rstride : 0));
	}
	if (inv)
		HIPCHK(ctx, launch_set_identity_rows(ctx->stream, ctx->dT + (size_t)(Np + Rp) * Np, Np, Np, nb, (long)ctx->T_stride));
	HIPCHK(ctx, hipMemsetAsync(ctx->dInfo, 0x7f, (size_t)nb * sizeof(int), ctx->stream));
	return GPEMU_OK;
}

static int enqueue_results(gpemu_ctx *ctx)
{
	const int Np = ctx->Np, Rp = ctx->Rp, nb = ctx->nb;
	HIPCHK(ctx, launch_gram_partials(ctx->stream, ctx->dT + (size_t)Np * Np, Np, Np, ctx->nrhs, Rp, ctx->dGramPart, nb,
	                                 (long)ctx->T_stride));
	HIPCHK(ctx, launch_finish(ctx->stream, ctx->dGramPart, Np / 64, Rp, ctx->nrhs, ctx->dT, Np, ctx->N, ctx->dRes, nb,
	                          (long)ctx->T_stride, (long)ctx->res_len));
	// the results land in the next slot of a pinned ring (RES_RING batches stay readable: a throughput caller collects
	// batch j while batches j+1 .. j+RES_RING-1 are in flight)
	ctx->res_seq++;
	ResSlot &s = ctx->newest();
	s.nb = nb;
	s.kind = 0;
	HIPCHK(ctx, hipMemcpyAsync(s.res, ctx->dRes, ((size_t)(nb - 1) * ctx->res_len + (size_t)Rp * Rp + 1) * sizeof(double),
	                           hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(s.info, ctx->dInfo, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipEventRecord(s.ev, ctx->stream));
	return GPEMU_OK;
}

// small dense Cholesky solve on the host (nreg x nreg): beta and Q = (H^T C^-1 H)^-1
// (regression.c:120-176 estimateBeta restated on the Gram matrix)
static bool small_chol_inverse(std::vector<double> &A, int n)
{
	for (int j = 0; j < n; j++) {
		double dsum = A[j * n + j];
		for (int k = 0; k < j; k++) dsum -= A[j * n + k] * A[j * n + k];
		if (!(dsum > 0.0)) return false;
		const double l = sqrt(dsum);
		A[j * n + j] = l;
		for (int i = j + 1; i < n; i++) {
			double s = A[i * n + j];
			for (int k = 0; k < j; k++) s -= A[i * n + k] * A[j * n + k];
			A[i * n + j] = s / l;
		}
	}
	// invert L, then A^-1 = L^-T L^-1
	std::vector<double> Li((size_t)n * n, 0.0);
	for (int c = 0; c < n; c++)
		for (int i = c; i < n; i++) {
			double s = (i == c) ? 1.0 : 0.0;
			for (int k = c; k < i; k++) s -= A[i * n + k] * Li[k * n + c];
			Li[i * n + c] = s / A[i * n + i];
		}
	for (int i = 0; i < n; i++)
		for (int j = 0; j < n; j++) {
			double s = 0.0;
			for (int k = std::max(i, j); k < n; k++) s += Li[k * n + i] * Li[k * n + j];
			A[i * n + j] = s;
		}
	return true;
}

struct HostLik { double yy, quad, sigma2, logdet; std::vector<double> beta, Q, Hy; int status; };

// from the results of one matrix (Gram matrix of [y|H] under C^-1, then log det C): element b of a ring slot
static HostLik host_likelihood(const gpemu_ctx *ctx, const ResSlot &s, int b = 0)
{
	HostLik r;
	const int Rp = ctx->Rp, nreg = ctx->nreg;
	const double *G = s.res + (size_t)b * ctx->res_len;
	r.logdet = G[Rp * Rp];
	r.yy = G[0];
	r.Hy.resize(nreg);
	r.Q.assign((size_t)nreg * nreg, 0.0);
	std::vector<double> HH((size_t)nreg * nreg);
	for (int a = 0; a < nreg; a++) {
		r.Hy[a] = G[(1 + a) * Rp];
		for (int b = 0; b < nreg; b++) HH[a * nreg + b] = G[(1 + a) * Rp + 1 + b];
	}
	r.Q = HH;
	r.beta.assign(nreg, NAN);
	r.quad = r.sigma2 = NAN;
	if (!small_chol_inverse(r.Q, nreg)) { r.status = GPEMU_ERR_REGRESSION; return r; }
	for (int a = 0; a < nreg; a++) {
		double s = 0.0;
		for (int b = 0; b < nreg; b++) s += r.Q[a * nreg + b] * r.Hy[b];
		r.beta[a] = s;
	}
	double bHy = 0.0, bHHb = 0.0;
	for (int a = 0; a < nreg; a++) {
		bHy += r.beta[a] * r.Hy[a];
		double s = 0.0;
		for (int b = 0; b < nreg; b++) s += HH[a * nreg + b] * r.beta[b];
		bHHb += r.beta[a] * s;
	}
	r.sigma2 = (r.yy - bHy) / (double)ctx->N;           // y.Cinv.(y - H beta)/N   (maxmultimin.c:259-263)
	r.quad = r.yy - 2.0 * bHy + bHHb;                   // r.Cinv.r               (estimator-fns.c:87-88)
	r.status = GPEMU_OK;
	return r;
}

// A batch of nb likelihood evaluations of the same model at nb theta vectors, factored in lock-step: every
// kernel of the factorisation handles all nb matrices (grid.y), so the latency-bound panel chain is paid once per
// batch and the trailing updates are nb times larger launches.  This is the device form of the reference's
// callEvalLhoodList (libRbind/rbind.c:626) and of the optimiser's independent restarts.
extern "C" int gpemu_loglik_batch_enqueue(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas)
{
	if (!ctx) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	if (nb < 1 || nb > GPEMU_MAX_BATCH) return fail(ctx, GPEMU_ERR_ARG, "batch size must be 1..GPEMU_MAX_BATCH");
	std::vector<CovParams> ps;
	int rc = make_cov_params_batch(ctx, nb, thetas, nthetas, &ps);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	rc = stage_matrices(ctx, ps.data(), nb, 0);
	if (rc) return rc;
	rc = run_potrf(ctx, 0);
	if (rc) return rc;
	invalidate_prediction(ctx);
	return enqueue_results(ctx);
}

// -log L as the reference writes it: its literal for log 2 pi (estimator-fns.c:48) and its order of operations
static double neg_loglik_of(const HostLik &r, int N)
{
	const double log_2_pi = 1.83788;
	return -1 * (-(1.0 / 2.0) * r.logdet - (N / 2.0) * log_2_pi + r.quad * (-1.0 / 2.0));
}

// element b of the batch in ring slot s (after its event or the stream has been waited for): the info word, then the host
// half of the likelihood.  Returns the element's status, the message set; GPEMU_ERR_NOT_PD leaves *r untouched
static int element_likelihood(gpemu_ctx *ctx, const ResSlot &s, int b, int *info, HostLik *r)
{
	const int inf = pivot_info(s.info[b]);
	if (info) *info = inf;
	if (inf) return fail(ctx, GPEMU_ERR_NOT_PD, "covariance matrix is not positive definite");
	*r = host_likelihood(ctx, s, b);
	return r->status ? fail(ctx, r->status, "H^T C^-1 H is not positive definite") : GPEMU_OK;
}

// results of element b of the batch in ring slot s.  After a regression failure logdet is still the matrix's, the rest NaN.
static int collect_one(gpemu_ctx *ctx, const ResSlot &s, int b, double *neg_loglik, double *sigma2, double *beta, double *logdet,
                       double *quad, int *info)
{
	HostLik r;
	const int st = element_likelihood(ctx, s, b, info, &r);
	const bool pd = st != GPEMU_ERR_NOT_PD;
	if (beta) for (int a = 0; a < ctx->nreg; a++) beta[a] = pd ? r.beta[a] : NAN;
	if (sigma2) *sigma2 = pd ? r.sigma2 : NAN;
	if (logdet) *logdet = pd ? r.logdet : NAN;
	if (quad) *quad = pd ? r.quad : NAN;
	if (neg_loglik) *neg_loglik = pd ? neg_loglik_of(r, ctx->N) : NAN;
	return st;
}

static void collect_batch(gpemu_ctx *ctx, const ResSlot &s, int nb, double *neg_loglik, double *sigma2, double *beta, double *logdet,
                          double *quad, int *info, int *status)
{
	for (int b = 0; b < nb; b++) {
		const int rc = collect_one(ctx, s, b, neg_loglik ? neg_loglik + b : nullptr, sigma2 ? sigma2 + b : nullptr,
		                           beta ? beta + (size_t)b * ctx->nreg : nullptr, logdet ? logdet + b : nullptr,
		                           quad ? quad + b : nullptr, info ? info + b : nullptr);
		if (status) status[b] = rc;
	}
}

extern "C" int gpemu_loglik_batch_collect(gpemu_ctx *ctx, int nb, double *neg_loglik, double *sigma2, double *beta,
                                          double *logdet, double *quad, int *info, int *status)
{
	if (!ctx) return GPEMU_ERR_ARG;
	if (nb < 1 || nb != ctx->nb) return fail(ctx, GPEMU_ERR_STATE, "batch size differs from the enqueued batch");
	if (!ctx->res_seq) return fail(ctx, GPEMU_ERR_STATE, "no such batch in the result ring");
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	collect_batch(ctx, ctx->newest(), nb, neg_loglik, sigma2, beta, logdet, quad, info, status);
	return GPEMU_OK;
}

// the batch enqueued `back` batches (of either kind) before the newest one (0 = newest), when it has nb elements and is of
// this kind (ResSlot::kind); otherwise nullptr, the message set (every such failure is a GPEMU_ERR_STATE)
static const ResSlot *ring_slot_back(gpemu_ctx *ctx, int back, int nb, int kind)
{
	auto no = [ctx](const char *msg) { fail(ctx, GPEMU_ERR_STATE, msg); return (const ResSlot *)nullptr; };
	if (back < 0 || back >= gpemu_ctx::RES_RING || (unsigned long long)back >= ctx->res_seq) return no("no such batch in the result ring");
	const ResSlot &s = ctx->ring[(ctx->res_seq - 1 - (unsigned long long)back) % gpemu_ctx::RES_RING];
	if (nb < 1 || nb != s.nb) return no("batch size differs from the enqueued batch");
	if (s.kind != kind)
		return no(kind ? "that batch is a likelihood batch: use gpemu_loglik_batch_collect_back"
		               : "that batch is a value+gradient batch: use gpemu_loglik_grad_batch_collect_back");
	return &s;
}

// results of the batch enqueued `back` batches before the newest one (0 = newest); waits for THAT batch only
extern "C" int gpemu_loglik_batch_collect_back(gpemu_ctx *ctx, int back, int nb, double *neg_loglik, double *sigma2,
                                               double *beta, double *logdet, double *quad, int *info, int *status)
{
	if (!ctx) return GPEMU_ERR_ARG;
	const ResSlot *s = ring_slot_back(ctx, back, nb, 0);
	if (!s) return GPEMU_ERR_STATE;
	HIPCHK(ctx, hipEventSynchronize(s->ev));
	collect_batch(ctx, *s, nb, neg_loglik, sigma2, beta, logdet, quad, info, status);
	return GPEMU_OK;
}

extern "C" int gpemu_loglik_batch(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas, double *neg_loglik,
                                  double *sigma2, double *beta, double *logdet, double *quad, int *info, int *status)
{
	int rc = gpemu_loglik_batch_enqueue(ctx, nb, thetas, nthetas);
	if (rc) return rc;
	return gpemu_loglik_batch_collect(ctx, nb, neg_loglik, sigma2, beta, logdet, quad, info, status);
}

extern "C" int gpemu_loglik_enqueue(gpemu_ctx *ctx, const double *thetas, int nthetas)
{
	if (!ctx) return GPEMU_ERR_ARG;
	return gpemu_loglik_batch_enqueue(ctx, 1, thetas, nthetas);
}

extern "C" int gpemu_loglik_collect(gpemu_ctx *ctx, double *neg_loglik, double *sigma2, double *beta, double *logdet,
                                    double *quad, int *info)
{
	if (!ctx) return GPEMU_ERR_ARG;
	if (ctx->nb != 1) return fail(ctx, GPEMU_ERR_STATE, "the enqueued work is a batch: use gpemu_loglik_batch_collect");
	if (!ctx->res_seq) return fail(ctx, GPEMU_ERR_STATE, "no such batch in the result ring");
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return collect_one(ctx, ctx->newest(), 0, neg_loglik, sigma2, beta, logdet, quad, info);
}

extern "C" int gpemu_loglik(gpemu_ctx *ctx, const double *thetas, int nthetas, double *neg_loglik, double *sigma2,
                            double *beta, double *logdet, double *quad, int *info)
{
	int rc = gpemu_loglik_enqueue(ctx, thetas, nthetas);
	if (rc) return rc;
	return gpemu_loglik_collect(ctx, neg_loglik, sigma2, beta, logdet, quad, info);
}

// ---------------------------------------------------------------------------
// covariance matrix / k vectors to host
// ---------------------------------------------------------------------------
extern "C" int gpemu_cov_matrix(gpemu_ctx *ctx, const double *thetas, int nthetas, double *c_out)
{
	if (!ctx || !c_out) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	CovParams p;
	int rc = make_cov_params(ctx, thetas, nthetas, &p);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = ctx->Np, N = ctx->N;
	DevBuf<double> buf;
	HIPCHK(ctx, buf.grow((size_t)Np * Np));
	HIPCHK(ctx, launch_cov_fill(ctx->stream, buf, Np, ctx->dX, N, Np, ctx->dX, N, Np, ctx->d, p, 0));
	HIPCHK(ctx, hipMemcpy2DAsync(c_out, (size_t)N * sizeof(double), buf, (size_t)Np * sizeof(double),
	                             (size_t)N * sizeof(double), N, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// k-vectors of M query rows (device) into out (Mp x Np, zero padded): Gram form when the hyper-parameters admit it
// (make_cov_params: p.gram) and the context was not told otherwise, else the difference form
static hipError_t fill_kvectors(gpemu_ctx *ctx, double *out, const double *xq_dev, int M, int Mp, const CovParams &p)
{
	if (p.gram && ctx->sched.kvec_gram && ctx->dXg && ctx->dMid)
		return launch_cov_kvec_gram(ctx->stream, out, ctx->Np, xq_dev, M, Mp, ctx->dX, ctx->dXg, ctx->dMid, ctx->N, ctx->Np, ctx->d, p);
	return launch_cov_fill(ctx->stream, out, ctx->Np, xq_dev, M, Mp, ctx->dX, ctx->N, ctx->Np, ctx->d, p, FILL_CLAMP);
}

extern "C" int gpemu_kvectors(gpemu_ctx *ctx, const double *thetas, int nthetas, int M, const double *xq, double *k_out)
{
	if (!ctx || !xq || !k_out || M < 1) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	CovParams p;
	int rc = make_cov_params(ctx, thetas, nthetas, &p);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = ctx->Np, N = ctx->N, Mp = round_up(M, 64);
	DevBuf<double> buf, dq;
	HIPCHK(ctx, buf.grow((size_t)Mp * Np));
	HIPCHK(ctx, dq.grow((size_t)M * ctx->d));
	HIPCHK(ctx, hipMemcpyAsync(dq, xq, (size_t)M * ctx->d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, fill_kvectors(ctx, buf, dq, M, Mp, p));
	HIPCHK(ctx, hipMemcpy2DAsync(k_out, (size_t)N * sizeof(double), buf, (size_t)Np * sizeof(double),
	                             (size_t)N * sizeof(double), M, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// prediction
// ---------------------------------------------------------------------------
static int factor_with_inverse(gpemu_ctx *ctx, const double *thetas, int nthetas, CovParams *p, int *info)
{
	int rc = make_cov_params(ctx, thetas, nthetas, p);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	rc = stage_matrices(ctx, p, 1, 1);
	if (rc) return rc;
	rc = run_potrf(ctx, 1);
	if (rc) return rc;
	rc = enqueue_results(ctx);
	if (rc) return rc;
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	const int inf = pivot_info(ctx->newest().info[0]);
	if (info) *info = inf;
	if (inf) return fail(ctx, GPEMU_ERR_NOT_PD, "covariance matrix is not positive definite");
	return GPEMU_OK;
}

// The prediction state of `dst` from element b of the factorisation (with inverse rows) that sits in `src`'s workspace and
// whose results have been collected (src == dst, b == 0: the single call).  Everything runs on src's stream, which is
// synchronised before the function returns; dst's own stream has nothing in flight (checked by the callers).
static int build_prediction_state(gpemu_ctx *src, int b, gpemu_ctx *dst, const CovParams &p, const HostLik &r, const double *thetas,
                                  int nthetas)
{
	const int Np = src->Np, Rp = src->Rp, nreg = src->nreg, N = src->N;
	const size_t la_rows = (size_t)Np + Rp;
	HIPCHK(src, dst->dLinvAug.grow(la_rows * Np));          // (made once per model: never moved under enqueued work)
	HIPCHK(src, dst->dBetaQ.grow((size_t)(nreg + nreg * nreg)));
	const double *Tb = src->dT + (size_t)b * src->T_stride;
	const double *Zt = Tb + (size_t)Np * Np;
	const double *U = Tb + (size_t)(Np + Rp) * Np;
	// rows [0,Np): L^-1 = U^T
	HIPCHK(src, launch_transpose(src->stream, dst->dLinvAug, Np, U, Np, Np));
	// (C^-1 [y|H])^T = Z^T U^T : rows Np.. of LinvAug used as scratch first
	GemmArgs g{};
	g.C = dst->dLinvAug + (size_t)Np * Np; g.ldc = Np;
	g.A = Zt; g.lda = Np;
	g.B = U; g.ldb = Np;
	g.m = Rp; g.n = Np; g.k0 = 0; g.k1 = Np; g.alpha = 1.0; g.beta = 0;
	HIPCHK(src, gemm(src, g));
	std::vector<double> cr((size_t)Rp * Np);
	HIPCHK(src, hipMemcpyAsync(cr.data(), dst->dLinvAug + (size_t)Np * Np, cr.size() * sizeof(double),
	                           hipMemcpyDeviceToHost, src->stream));
	HIPCHK(src, hipStreamSynchronize(src->stream));
	// row 0 <- gamma = C^-1 y - (C^-1 H) beta = C^-1 (y - H beta); rows 1.. keep W^T = (C^-1 H)^T
	for (int j = 0; j < Np; j++) {
		double s = cr[j];
		for (int a = 0; a < nreg; a++) s -= r.beta[a] * cr[(size_t)(1 + a) * Np + j];
		cr[j] = (j < N) ? s : 0.0;
	}
	for (int a = src->nrhs; a < Rp; a++)
		for (int j = 0; j < Np; j++) cr[(size_t)a * Np + j] = 0.0;
	HIPCHK(src, hipMemcpyAsync(dst->dLinvAug + (size_t)Np * Np, cr.data(), cr.size() * sizeof(double),
	                           hipMemcpyHostToDevice, src->stream));
	std::vector<double> bq(nreg + (size_t)nreg * nreg);
	for (int a = 0; a < nreg; a++) bq[a] = r.beta[a];
	for (int a = 0; a < nreg * nreg; a++) bq[nreg + a] = r.Q[a];
	HIPCHK(src, hipMemcpyAsync(dst->dBetaQ, bq.data(), bq.size() * sizeof(double), hipMemcpyHostToDevice, src->stream));
	HIPCHK(src, hipStreamSynchronize(src->stream));
	dst->h_beta = r.beta; dst->h_Q = r.Q;
	dst->pred_cov = p;
	dst->kappa = p.amp + p.nug;                       // cov(x*,x*): emulator_struct.c:135 (nugget included)
	dst->pred_ready = true;
	dst->cinv_ready = false;
	dst->linvT_ready = false;
	dst->pred_serial++;                               // (gpemu_design_gain: what it keeps belongs to one set-up)
	dst->last_thetas.assign(thetas, thetas + nthetas);
	return GPEMU_OK;
}

extern "C" int gpemu_predict_setup(gpemu_ctx *ctx, const double *thetas, int nthetas, double *beta_out, int *info)
{
	if (!ctx) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	invalidate_prediction(ctx);
	CovParams p;
	int rc = factor_with_inverse(ctx, thetas, nthetas, &p, info);
	if (rc) return rc;
	HostLik r = host_likelihood(ctx, ctx->newest());
	if (r.status) return fail(ctx, r.status, "H^T C^-1 H is not positive definite");
	rc = build_prediction_state(ctx, 0, ctx, p, r, thetas, nthetas);
	if (rc) return rc;
	ctx->fact_in_T = true;
	if (beta_out) for (int a = 0; a < ctx->nreg; a++) beta_out[a] = r.beta[a];
	return GPEMU_OK;
}

// alloc_multi_emulator (multivar_support.c:30-52) loops alloc_emulator_struct over the nr PCA components of a multi-output
// model: same design, covariance function and regression order, a training vector and thetas of its own each.  Here the nr
// factorisations with their inverse rows run as ONE lock-step batch in the first context's workspace (blockIdx.y = component,
// every component under its own right-hand-side rows), and each context receives its own prediction state; afterwards the
// contexts answer queries on their own streams as if gpemu_predict_setup had been called on each -- with the same bits: an
// element of a lock-step batch is the evaluation done alone.
extern "C" int gpemu_predict_setup_batch(gpemu_ctx *const *ctxs, int n, const double *thetas, int nthetas, double *beta_out, int *info,
                                         int *status)
{
	if (!ctxs || n < 1 || !ctxs[0]) return GPEMU_ERR_ARG;
	gpemu_ctx *lead = ctxs[0];
	if (n > GPEMU_MAX_BATCH) return fail(lead, GPEMU_ERR_ARG, "at most GPEMU_MAX_BATCH components per call");
	if (!lead->dX) return fail(lead, GPEMU_ERR_STATE, "model not set");
	for (int c = 0; c < n; c++) {
		gpemu_ctx *x = ctxs[c];
		if (!x || !x->dX) return fail(lead, GPEMU_ERR_STATE, "model not set in every context");
		for (int e = 0; e < c; e++) if (ctxs[e] == x) return fail(lead, GPEMU_ERR_ARG, "the same context twice");
		if (x->device != lead->device || x->kind != lead->kind || x->order != lead->order || x->N != lead->N || x->d != lead->d ||
		    x->mode != lead->mode || x->hX != lead->hX)
			return fail(lead, GPEMU_ERR_ARG, "the contexts of a batched set-up share device, design, covariance function, regression order and modes");
		if (x->pred_pending.kind != PRED_NONE) return fail(lead, GPEMU_ERR_STATE, "a prediction batch is enqueued in one of the contexts: collect it first");
	}
	// (only now: a call refused above leaves every context as it was, the ones listed before the offending one too)
	for (int c = 0; c < n; c++) invalidate_prediction(ctxs[c]);
	std::vector<CovParams> ps;
	if (const int rc = make_cov_params_batch(lead, n, thetas, nthetas, &ps)) return rc;
	HIPCHK(lead, hipSetDevice(lead->device));
	const int Np = lead->Np, Rp = lead->Rp, nreg = lead->nreg;
	// the components' right-hand-side rows [y_c | H]^T side by side (each context built its own at gpemu_set_model /
	// gpemu_set_training, synchronously)
	{
		DevBuf<double> rr;                             // (released when the batch has been factored)
		const size_t rlen = (size_t)Rp * Np;
		HIPCHK(lead, rr.grow((size_t)n * rlen));
		for (int c = 0; c < n; c++)
			HIPCHK(lead, hipMemcpyAsync(rr + (size_t)c * rlen, ctxs[c]->dRrows, rlen * sizeof(double), hipMemcpyDeviceToDevice, lead->stream));
		int rc = stage_matrices(lead, ps.data(), n, 1, rr, (long)rlen);
		if (!rc) rc = run_potrf(lead, 1);
		if (!rc) rc = enqueue_results(lead);
		if (rc) return rc;
		HIPCHK(lead, hipStreamSynchronize(lead->stream));
	}
	const ResSlot &res = lead->newest();               // the batch just factored
	int worst = GPEMU_OK;
	for (int c = 0; c < n; c++) {
		const int inf = pivot_info(res.info[c]);
		if (info) info[c] = inf;
		int st = GPEMU_OK;
		if (inf) st = GPEMU_ERR_NOT_PD;
		else {
			HostLik r = host_likelihood(lead, res, c);
			if (r.status) st = r.status;
			else {
				st = build_prediction_state(lead, c, ctxs[c], ps[c], r, thetas + (size_t)c * nthetas, nthetas);
				ctxs[c]->fact_in_T = (c == 0);                // (element 0 of the batch sits where a single set-up leaves it)
				if (st == GPEMU_OK && beta_out) for (int a = 0; a < nreg; a++) beta_out[(size_t)c * nreg + a] = r.beta[a];
			}
		}
		if (status) status[c] = st;
		if (st != GPEMU_OK && worst == GPEMU_OK) worst = st;
	}
	if (worst == GPEMU_ERR_NOT_PD) return fail(lead, worst, "covariance matrix is not positive definite");
	if (worst == GPEMU_ERR_REGRESSION) return fail(lead, worst, "H^T C^-1 H is not positive definite");
	return worst;
}

// Everything a process pays once before its first result -- the HIP runtime, the device's code objects (loaded at the first
// launch from each of this library's translation units), the exp and tile tables -- on a throw-away context with a 64-point
// model: one evaluation, one prediction set-up, one prediction.  Meant for a thread of its own while the caller is still
// reading its input (csrc/host: gpemu_host_warm_start).
extern "C" int gpemu_warm_start(int device)
{
	gpemu_ctx *ctx = nullptr;
	int rc = gpemu_ctx_create(&ctx, device);
	if (rc) return rc;
	const int N = 64, d = 2;
	std::vector<double> X((size_t)N * d), y(N);
	for (int i = 0; i < N; i++) {
		X[(size_t)i * d] = (i % 8) / 8.0 + 0.01 * i;
		X[(size_t)i * d + 1] = (i / 8) / 8.0;
		y[i] = std::sin(0.3 * i);
	}
	{
		// (one covariance function is enough: the instantiations for the others sit in the same code objects)
		const double th[4] = {0.0, -3.0, -1.0, -1.0};
		rc = gpemu_set_model(ctx, GPEMU_POWEREXP, 1, N, d, X.data(), y.data());
		double v, s2, m, var;
		int info = 0;
		if (!rc) rc = gpemu_loglik(ctx, th, 4, &v, &s2, nullptr, nullptr, nullptr, &info);
		if (!rc) rc = gpemu_predict_setup(ctx, th, 4, nullptr, &info);
		if (!rc) rc = gpemu_predict_batch(ctx, 1, X.data(), &m, &var);
	}
	gpemu_ctx_destroy(ctx);
	return rc;
}

constexpr int PRED_SPLIT_MAX = 16;

static int ensure_pred_batch(gpemu_ctx *ctx, int mb)
{
	const int rc = grow(ctx, ctx->dKq, (size_t)mb * ctx->Np);
	if (rc) return rc;
	// V also holds the split-K partial products of small batches: PRED_SPLIT_MAX slices of up to 128 query rows
	return grow(ctx, ctx->dV, (size_t)std::max(mb, 128 * PRED_SPLIT_MAX) * (ctx->Np + ctx->Rp));
}

constexpr int PRED_BATCH_MAX = 16384;

// V = Kq LinvAug^T for the mb query rows in dKq: Np columns against the triangular rows of L^-1, then Rp against gamma and W^T
// (gpemu_predict_batch_dev and gpemu_predict_var_grad_dev).  The schedule switches are applied here already -- gemm() does it
// again -- for the tile-shape question of launch_aug_product and the callers' own questions about the call.
static GemmArgs aug_product_args(gpemu_ctx *ctx, int mb)
{
	const int Np = ctx->Np, Rp = ctx->Rp;
	GemmArgs g{};
	g.C = ctx->dV; g.ldc = Np + Rp;
	g.A = ctx->dKq; g.lda = Np;
	g.B = ctx->dLinvAug; g.ldb = Np;
	g.m = mb; g.n = Np + Rp; g.k0 = 0; g.k1 = Np; g.alpha = 1.0; g.beta = 0;
	g.kend_mode = 1; g.kend_off = 0;
	apply_sched(ctx->sched, g);
	return g;
}

// launches what aug_product_args made (the caller may have split K since)
static hipError_t launch_aug_product(gpemu_ctx *ctx, const GemmArgs &g)
{
	if (g.ksplit <= 1 && ctx->sched.split_rhs_rows && gemm_uses_big_tiles(g)) {
		// 128x128 tiles: the 64 columns of gamma and W^T behind the Np triangular ones would make a 65th tile column that is
		// half empty at the full contraction length (1.5 % of the sweep's tile time): they go to a 64x64-tile launch of
		// their own, as the right-hand-side rows of the factorisation's updates do.  Same chain per element, same bits.
		const int Np = ctx->Np;
		GemmArgs a = g;
		a.n = Np;
		const hipError_t e = gemm(ctx, a);
		if (e != hipSuccess) return e;
		GemmArgs b = g;
		b.C = ctx->dV + Np; b.B = ctx->dLinvAug + (size_t)Np * Np;
		b.n = ctx->Rp; b.kend_mode = 0; b.force_cfg = 2;
		return gemm(ctx, b);
	}
	return gemm(ctx, g);
}

// what the fused sweeps read of the model besides dX: the design centred per dimension with its centres where the model has
// them (else as given, mid = NULL), the gamma row of dLinvAug, and whether the k-vectors are taken in Gram form
struct SweepInputs {
	const double *Xc, *mid, *gamma;
	bool gram;
};

static SweepInputs sweep_inputs(gpemu_ctx *ctx)
{
	const bool centred = ctx->dXg && ctx->dMid;
	SweepInputs s;
	s.Xc = centred ? (const double *)ctx->dXg : (const double *)ctx->dX;
	s.mid = centred ? (const double *)ctx->dMid : nullptr;
	s.gamma = ctx->dLinvAug + (size_t)ctx->Np * ctx->Np;
	s.gram = ctx->pred_cov.gram && ctx->sched.kvec_gram && centred;
	return s;
}

extern "C" int gpemu_predict_batch_dev(gpemu_ctx *ctx, int M, const double *xq_dev, double *mean_dev, double *var_dev)
{
	if (!ctx || M < 1 || !xq_dev || !mean_dev || !var_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = ctx->Np, Rp = ctx->Rp, N = ctx->N, d = ctx->d;
	const int cap = std::min(PRED_BATCH_MAX, round_up(M, 64));
	int rc = ensure_pred_batch(ctx, cap);
	if (rc) return rc;
	for (int q0 = 0; q0 < M; q0 += cap) {
		const int mb = std::min(cap, M - q0);
		const int mbp = round_up(mb, 64);
		GemmArgs g = aug_product_args(ctx, mb);
		// a few queries (emulate_point: ONE) give one or two tile rows with K = N each: split K over the chip
		// (0.46 -> 0.1 ms per call at N=8192); the slices are summed in order by the finishing kernel
		int nslice = 1;
		{
			const long tiles = (long)(mbp / 64) * ((Np + Rp + 63) / 64);      // 64x64 tiles of the unsplit product
			if (tiles < 1024) nslice = (int)std::max(1L, std::min((long)std::min(PRED_SPLIT_MAX, Np / 512), 2048 / tiles));
			if ((long)nslice * mbp > 128L * PRED_SPLIT_MAX) nslice = 1;       // capacity of dV for the partial products
		}
		// up to 16 queries with a long contraction (emulate_point: ONE query): the few-queries path -- a one-thread-per-design-
		// point k-vector kernel, the skinny split-K product, an epilogue with the slice sums fused in (three launches; the batch
		// kernels would set up their tables and tiles for 63 padding rows: 16 + 93 + 6 + 20 us of kernels at N = 8192)
		const bool few = mb <= 16 && nslice > 1;
		if (!few) {
			ProfScope ps(ctx, GPEMU_PROF_FILL, 0.0, 8.0 * (double)mbp * Np);
			HIPCHK(ctx, fill_kvectors(ctx, ctx->dKq, xq_dev + (size_t)q0 * d, mb, mbp, ctx->pred_cov));
		} else {
			HIPCHK(ctx, launch_kvec_small(ctx->stream, ctx->dKq, Np, xq_dev + (size_t)q0 * d, mb, ctx->dX, N, Np, d, ctx->pred_cov));
		}
		if (nslice > 1) { g.ksplit = nslice; g.bsC = (long)mbp * (Np + Rp); }
		if (few) {
			// up to 16 queries (emulate_point: one): the skinny kernel, one 16-row query tile, instead of 64-row GEMM
			// tiles (97 vs 115 us at N=8192; from 17 queries on the split-K GEMM is as fast)
			const int klen = (((Np + nslice - 1) / nslice) + 15) & ~15;
			// (the count walks the Np + Rp columns on the host: only for a profile, as in gemm())
			ProfScope ps(ctx, GPEMU_PROF_GEMM, prof_on(ctx, GPEMU_PROF_GEMM) ? gemm_flops(g) : 0.0, 0.0);
			if (mb == 1 && ctx->sched.gemv_point)
				// ONE query: a matrix-vector stream over whole rows of L^-1 instead of the matrix unit's 16-row reads
				HIPCHK(ctx, launch_gemv_tri(ctx->stream, ctx->dKq, Np, ctx->dLinvAug, Np, ctx->dV, Np + Rp, (long)mbp * (Np + Rp),
				                            1, Np + Rp, Np, Np, nslice, klen));
			else
			HIPCHK(ctx, launch_skinny_nt(ctx->stream, ctx->dKq, Np, ctx->dLinvAug, Np, ctx->dV, Np + Rp, (long)mbp * (Np + Rp),
			                             1, Np + Rp, Np, Np, nslice, klen));
			HIPCHK(ctx, launch_predict_finish_small(ctx->stream, ctx->dV, Np + Rp, (long)mbp * (Np + Rp), nslice, mb, Np, ctx->nreg, d,
			                                        xq_dev + (size_t)q0 * d, ctx->dBetaQ, ctx->kappa, mean_dev + q0, var_dev + q0));
			continue;
		}
		HIPCHK(ctx, launch_aug_product(ctx, g));
		HIPCHK(ctx, launch_predict_finish(ctx->stream, ctx->dV, Np + Rp, mb, Np, ctx->nreg, ctx->order, d,
		                                  xq_dev + (size_t)q0 * d, ctx->dBetaQ, ctx->kappa, mean_dev + q0, var_dev + q0,
		                                  nslice, (long)mbp * (Np + Rp)));
	}
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// mean-only sweep (gpemu.h): two launches per block of up to PRED_BATCH_MAX queries on the context's stream -- the fused
// k-vector . gamma kernel and the slice sum with h^T beta.  Reads dX, dXg, dMid, the gamma row of dLinvAug and dBetaQ; its
// only scratch is dMeanPart.  dKq and dV are neither read nor allocated.
// ---------------------------------------------------------------------------
extern "C" int gpemu_predict_mean_dev(gpemu_ctx *ctx, int M, const double *xq_dev, double *mean_dev)
{
	if (!ctx || M < 1 || !xq_dev || !mean_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = ctx->Np, N = ctx->N, d = ctx->d;
	const int nslice = predict_mean_slices(Np);
	const int cap = std::min(PRED_BATCH_MAX, round_up(M, 64));
	// (laid out with the row length it was sized for: a later, shorter call uses the same stride)
	int rc = grow(ctx, ctx->dMeanPart, (size_t)nslice * cap);
	if (rc) return rc;
	const long pstride = (long)(ctx->dMeanPart.size() / (size_t)nslice);
	const CovParams &p = ctx->pred_cov;
	const SweepInputs in = sweep_inputs(ctx);        // (the kernel takes dXg and dMid as they are: it reads them in Gram form only)
	for (int q0 = 0; q0 < M; q0 += cap) {
		const int mb = std::min(cap, M - q0);
		const double *xq = xq_dev + (size_t)q0 * d;
		if (prof_on(ctx, GPEMU_PROF_MEAN)) { ctx->prof.tag.push_back("predict_mean"); ctx->prof.tag.push_back("predict_mean_finish"); }
		{
			// flops: per element the squared distance (3 d) and the product with gamma (2); bytes: coordinates in, mean out
			ProfScope ps(ctx, GPEMU_PROF_MEAN, (double)mb * N * (3.0 * d + 2.0), 8.0 * (double)mb * (d + 1));
			HIPCHK(ctx, launch_predict_mean(ctx->stream, ctx->dMeanPart, pstride, xq, mb, ctx->dX, ctx->dXg, ctx->dMid, in.gamma, N, Np, d, p, in.gram));
		}
		{
			ProfScope ps(ctx, GPEMU_PROF_MEAN, 2.0 * mb * ctx->nreg, 0.0);
			HIPCHK(ctx, launch_predict_mean_finish(ctx->stream, ctx->dMeanPart, pstride, nslice, mb, ctx->nreg, d, xq, ctx->dBetaQ,
			                                       mean_dev + q0));
		}
	}
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// mean and its gradient with respect to the query point (gpemu.h): two launches per block of up to
// PRED_BATCH_MAX queries -- the fused sweep (k tile as weights times gamma [1, x - mid] on the matrix unit) and the slice sum
// with the regression term.  Reads what the mean-only sweep reads; scratch and staging are its own (dMGradPart, dMGrad,
// hMGrad beside the shared coordinate / mean staging); dKq, dV and dMeanPart are not touched.
// ---------------------------------------------------------------------------
extern "C" int gpemu_predict_mean_grad_dev(gpemu_ctx *ctx, int M, const double *xq_dev, double *mean_dev, double *grad_dev)
{
	if (!ctx || M < 1 || !xq_dev || !grad_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = ctx->Np, N = ctx->N, d = ctx->d;
	const int nslice = predict_mean_slices(Np), pw = predict_mean_grad_width(d);
	const int cap = std::min(PRED_BATCH_MAX, round_up(M, 64));
	int rc = grow(ctx, ctx->dMGradPart, (size_t)nslice * cap * (size_t)(1 + pw));
	if (rc) return rc;
	// (laid out with the row count it was sized for: a later, shorter call uses the same strides)
	const long pstride = (long)(ctx->dMGradPart.size() / ((size_t)nslice * (size_t)(1 + pw)));
	double *mpart = ctx->dMGradPart, *gpart = mpart + (size_t)nslice * pstride;
	const CovParams &p = ctx->pred_cov;
	const SweepInputs in = sweep_inputs(ctx);
	for (int q0 = 0; q0 < M; q0 += cap) {
		const int mb = std::min(cap, M - q0);
		const double *xq = xq_dev + (size_t)q0 * d;
		if (prof_on(ctx, GPEMU_PROF_MEAN_GRAD)) { ctx->prof.tag.push_back("predict_mean_grad"); ctx->prof.tag.push_back("predict_mean_grad_finish"); }
		{
			// flops: per element the squared distance (3 d), the product with gamma (2) and the 1 + d columns of the second
			// product (2 each); bytes: coordinates in, mean and gradient out
			ProfScope ps(ctx, GPEMU_PROF_MEAN_GRAD, (double)mb * N * (3.0 * d + 2.0 + 2.0 * (d + 1)), 8.0 * (double)mb * (2 * d + 1));
			HIPCHK(ctx, launch_predict_mean_grad(ctx->stream, mpart, gpart, pstride, xq, mb, ctx->dX, in.Xc, in.mid, in.gamma, N, Np, d, p, in.gram));
		}
		{
			ProfScope ps(ctx, GPEMU_PROF_MEAN_GRAD, 2.0 * mb * ctx->nreg + 4.0 * mb * d, 0.0);
			HIPCHK(ctx, launch_predict_mean_grad_finish(ctx->stream, mpart, gpart, pstride, nslice, mb, ctx->nreg, d, xq, in.mid, ctx->dBetaQ, p,
			                                            mean_dev ? mean_dev + q0 : nullptr, grad_dev + (size_t)q0 * d));
		}
	}
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// mean, variance and the variance's gradient with respect to the query point (gpemu.h).  Per block of up to
// PRED_BATCH_MAX queries: the k-vectors and V = Kq LinvAug^T as in gpemu_predict_batch_dev (K never split: the u rows must be
// whole), the finish, Q r per query into V's columns Np .., the second product A^T = LinvAugT [u | Q r]^T into dKq (its
// k-vectors are dead by then; row starts skipped: L^-T is upper triangular), the fused sweep and its finish.  Uses dKq and dV
// -- unlike the mean sweeps --, its own dVGradPart and, made by the first call after a set-up, dLinvAugT.
// ---------------------------------------------------------------------------
static int ensure_linv_transposed(gpemu_ctx *ctx)
{
	if (ctx->linvT_ready) return GPEMU_OK;
	const int Np = ctx->Np, Rp = ctx->Rp;
	const long ldt = (long)Np + Rp;
	const int rc = grow(ctx, ctx->dLinvAugT, (size_t)Np * ldt, false, "out of device memory for the transposed copy of L^-1 (8 Np (Np + Rp) bytes)");
	if (rc) return rc;
	HIPCHK(ctx, launch_transpose(ctx->stream, ctx->dLinvAugT, ldt, ctx->dLinvAug, Np, Np));
	HIPCHK(ctx, launch_transpose_rect(ctx->stream, ctx->dLinvAugT + Np, ldt, ctx->dLinvAug + (size_t)Np * Np, Np, Rp, Np));
	ctx->linvT_ready = true;
	return GPEMU_OK;
}

extern "C" int gpemu_predict_var_grad_dev(gpemu_ctx *ctx, int M, const double *xq_dev, double *mean_dev, double *var_dev, double *grad_dev)
{
	if (!ctx || M < 1 || !xq_dev || !grad_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = ctx->Np, Rp = ctx->Rp, N = ctx->N, d = ctx->d;
	const int nslice = predict_mean_slices(Np), pw = predict_mean_grad_width(d);
	const int cap = std::min(PRED_BATCH_MAX, round_up(M, 64));
	int rc = ensure_pred_batch(ctx, cap);
	if (!rc) rc = grow(ctx, ctx->dVGradPart, (size_t)nslice * cap * (size_t)pw + 2 * (size_t)cap);
	if (!rc) rc = ensure_linv_transposed(ctx);
	if (rc) return rc;
	double *gpart = ctx->dVGradPart, *spare = gpart + (size_t)nslice * cap * (size_t)pw;
	const long ldv = (long)Np + Rp;
	const CovParams &p = ctx->pred_cov;
	const SweepInputs in = sweep_inputs(ctx);
	for (int q0 = 0; q0 < M; q0 += cap) {
		const int mb = std::min(cap, M - q0);
		const int mbp = round_up(mb, 64);
		const double *xq = xq_dev + (size_t)q0 * d;
		{
			ProfScope ps(ctx, GPEMU_PROF_FILL, 0.0, 8.0 * (double)mbp * Np);
			HIPCHK(ctx, fill_kvectors(ctx, ctx->dKq, xq, mb, mbp, p));
		}
		HIPCHK(ctx, launch_aug_product(ctx, aug_product_args(ctx, mb)));
		HIPCHK(ctx, launch_predict_finish(ctx->stream, ctx->dV, ldv, mb, Np, ctx->nreg, ctx->order, d, xq, ctx->dBetaQ, ctx->kappa,
		                                  mean_dev ? mean_dev + q0 : spare, var_dev ? var_dev + q0 : spare + cap, 1, (long)mbp * ldv));
		HIPCHK(ctx, launch_predict_qr(ctx->stream, ctx->dV, ldv, mb, Np, Rp, ctx->nreg, d, xq, ctx->dBetaQ));
		// A^T (Np x mbp) = LinvAugT (Np x (Np + Rp), row i zero before column i) . V^T
		GemmArgs t{};
		t.C = ctx->dKq; t.ldc = mbp;
		t.A = ctx->dLinvAugT; t.lda = ldv;
		t.B = ctx->dV; t.ldb = ldv;
		t.m = Np; t.n = mb; t.k0 = 0; t.k1 = Np + Rp; t.alpha = 1.0; t.beta = 0;
		t.kstart_mode = 1; t.kstart_off = 0;
		HIPCHK(ctx, gemm(ctx, t));
		if (prof_on(ctx, GPEMU_PROF_VAR_GRAD)) { ctx->prof.tag.push_back("predict_var_grad"); ctx->prof.tag.push_back("predict_var_grad_finish"); }
		{
			// flops: per element the squared distance (3 d), the product with a (1) and the 1 + d columns of the matrix
			// product (2 each); bytes: A^T and the coordinates in, the gradient out
			ProfScope ps(ctx, GPEMU_PROF_VAR_GRAD, (double)mb * N * (3.0 * d + 1.0 + 2.0 * (d + 1)), 8.0 * (double)mb * (N + 2 * d));
			HIPCHK(ctx, launch_predict_var_grad(ctx->stream, gpart, cap, xq, mb, ctx->dX, in.Xc, in.mid, ctx->dKq, mbp, N, Np, d, p, in.gram));
		}
		{
			ProfScope ps(ctx, GPEMU_PROF_VAR_GRAD, 2.0 * mb * d * (nslice + 3.0), 0.0);
			HIPCHK(ctx, launch_predict_var_grad_finish(ctx->stream, gpart, cap, nslice, mb, ctx->nreg, d, xq, in.mid, ctx->dV, ldv, Np, p,
			                                           grad_dev + (size_t)q0 * d));
		}
	}
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// host-buffer entries of the four kinds above, in two halves each: the queries are staged through pinned memory, the kind's
// _dev entry runs on the context's stream and the results come back into pinned memory; nothing blocks until the collect.
// Several contexts (the PCA components of a multi-output emulator) can so work on one query at the same time.  One batch of
// any kind is pending per context (ctx->pred_pending); only the collect of its own kind takes it.
// ---------------------------------------------------------------------------
// the staging every kind uses (coordinates, means, variances), for at least M queries
static int ensure_pred_stage(gpemu_ctx *ctx, int M)
{
	if (ctx->stage_cap() >= (size_t)M) return GPEMU_OK;
	const int d = ctx->d;
	const size_t cap = (size_t)std::max(M, 64);
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->hStage.reset();                           // (the capacity is zero until all three are there again)
	int rc = grow(ctx, ctx->dXq, cap * d);
	if (!rc) rc = grow(ctx, ctx->dMean, 2 * cap);
	if (rc) return rc;
	HIPCHK(ctx, ctx->hStage.grow(cap * (d + 2)));
	return GPEMU_OK;
}

// the gradient staging of the two gradient kinds, for at least M queries
static int ensure_pred_grad_stage(gpemu_ctx *ctx, int M)
{
	if (ctx->mgrad_cap() >= (size_t)M) return GPEMU_OK;
	const size_t gcap = (size_t)std::max(M, 64);
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->hMGrad.reset();
	if (const int rc = grow(ctx, ctx->dMGrad, gcap * ctx->d)) return rc;
	HIPCHK(ctx, ctx->hMGrad.grow(gcap * ctx->d));
	return GPEMU_OK;
}

// per PredKind: what the kind stages back to the host besides the means, which every kind does; which outputs its collect
// refuses to go without (the others may be NULL); its name and its collect function for the error texts
struct PredKindInfo {
	bool var, grad;
	bool need_mean, need_var, need_grad;
	const char *name, *collect;
};
static constexpr PredKindInfo PRED_KINDS[] = {
	{false, false, false, false, false, "", ""},                                              // PRED_NONE
	{true, false, true, true, false, "mean+variance", "gpemu_predict_batch_collect"},         // PRED_MEAN_VAR
	{false, false, true, false, false, "mean-only", "gpemu_predict_mean_collect"},            // PRED_MEAN
	{false, true, false, false, true, "mean-gradient", "gpemu_predict_mean_grad_collect"},    // PRED_MEAN_GRAD
	{true, true, false, false, true, "variance-gradient", "gpemu_predict_var_grad_collect"},  // PRED_VAR_GRAD
};

static bool pred_outputs_ok(PredKind kind, const double *mean, const double *var, const double *grad)
{
	const PredKindInfo &k = PRED_KINDS[kind];
	return (mean || !k.need_mean) && (var || !k.need_var) && (grad || !k.need_grad);
}

static int pred_enqueue(gpemu_ctx *ctx, PredKind kind, int M, const double *xq)
{
	if (!ctx || kind == PRED_NONE || M < 1 || !xq) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->pred_pending.kind != PRED_NONE) return fail(ctx, GPEMU_ERR_STATE, "a prediction batch is already enqueued: collect it first");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const PredKindInfo &k = PRED_KINDS[kind];
	const int d = ctx->d;
	int rc = ensure_pred_stage(ctx, M);
	if (!rc && k.grad) rc = ensure_pred_grad_stage(ctx, M);
	if (rc) return rc;
	const size_t cap = ctx->stage_cap();
	double *hx = ctx->hStage, *hm = hx + cap * d, *hv = hm + cap;
	memcpy(hx, xq, (size_t)M * d * sizeof(double));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dXq, hx, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	switch (kind) {
	case PRED_MEAN_VAR: rc = gpemu_predict_batch_dev(ctx, M, ctx->dXq, ctx->dMean, ctx->dVar()); break;
	case PRED_MEAN: rc = gpemu_predict_mean_dev(ctx, M, ctx->dXq, ctx->dMean); break;
	case PRED_MEAN_GRAD: rc = gpemu_predict_mean_grad_dev(ctx, M, ctx->dXq, ctx->dMean, ctx->dMGrad); break;
	case PRED_VAR_GRAD: rc = gpemu_predict_var_grad_dev(ctx, M, ctx->dXq, ctx->dMean, ctx->dVar(), ctx->dMGrad); break;
	case PRED_NONE: break;                           // (refused above; here for the compiler's list of cases)
	}
	if (rc) return rc;
	if (k.var && cap <= 1024) {
		// ONE copy for a small batch, which keeps the latency of a single query low: hm | hv on the host and dMean | dVar on
		// the device have the same layout, cap entries apart
		HIPCHK(ctx, hipMemcpyAsync(hm, ctx->dMean, (cap + M) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	} else {
		HIPCHK(ctx, hipMemcpyAsync(hm, ctx->dMean, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
		if (k.var) HIPCHK(ctx, hipMemcpyAsync(hv, ctx->dVar(), (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	}
	if (k.grad) HIPCHK(ctx, hipMemcpyAsync(ctx->hMGrad, ctx->dMGrad, (size_t)M * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	ctx->pred_pending = {kind, M};
	return GPEMU_OK;
}

// a refused collect, for whatever reason, leaves the batch pending
static int pred_collect(gpemu_ctx *ctx, PredKind kind, int M, double *mean, double *var, double *grad)
{
	if (!ctx || !pred_outputs_ok(kind, mean, var, grad)) return GPEMU_ERR_ARG;
	const PredPending pend = ctx->pred_pending;
	if (pend.kind == PRED_NONE || M != pend.M) return fail(ctx, GPEMU_ERR_STATE, "no enqueued prediction batch of this size");
	if (pend.kind != kind) {
		char buf[160];
		snprintf(buf, sizeof buf, "the enqueued batch is a %s batch: collect it with %s", PRED_KINDS[pend.kind].name, PRED_KINDS[pend.kind].collect);
		return fail(ctx, GPEMU_ERR_STATE, buf);
	}
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	// (an output the kind does not have is NULL: the wrappers below pass it so)
	const double *hm = ctx->hStage + ctx->stage_cap() * ctx->d, *hv = hm + ctx->stage_cap();
	if (mean) memcpy(mean, hm, (size_t)M * sizeof(double));
	if (var) memcpy(var, hv, (size_t)M * sizeof(double));
	if (grad) memcpy(grad, ctx->hMGrad, (size_t)M * ctx->d * sizeof(double));
	ctx->pred_pending = {};
	return GPEMU_OK;
}

// both halves in one call (the outputs are looked at first: nothing is enqueued that the collect would then refuse)
static int pred_sync(gpemu_ctx *ctx, PredKind kind, int M, const double *xq, double *mean, double *var, double *grad)
{
	if (!pred_outputs_ok(kind, mean, var, grad)) return GPEMU_ERR_ARG;
	const int rc = pred_enqueue(ctx, kind, M, xq);
	return rc ? rc : pred_collect(ctx, kind, M, mean, var, grad);
}

extern "C" int gpemu_predict_batch_enqueue(gpemu_ctx *ctx, int M, const double *xq) { return pred_enqueue(ctx, PRED_MEAN_VAR, M, xq); }
extern "C" int gpemu_predict_batch_collect(gpemu_ctx *ctx, int M, double *mean, double *var) { return pred_collect(ctx, PRED_MEAN_VAR, M, mean, var, nullptr); }
extern "C" int gpemu_predict_batch(gpemu_ctx *ctx, int M, const double *xq, double *mean, double *var)
{
	return pred_sync(ctx, PRED_MEAN_VAR, M, xq, mean, var, nullptr);
}

extern "C" int gpemu_predict_mean_enqueue(gpemu_ctx *ctx, int M, const double *xq) { return pred_enqueue(ctx, PRED_MEAN, M, xq); }
extern "C" int gpemu_predict_mean_collect(gpemu_ctx *ctx, int M, double *mean) { return pred_collect(ctx, PRED_MEAN, M, mean, nullptr, nullptr); }
extern "C" int gpemu_predict_mean(gpemu_ctx *ctx, int M, const double *xq, double *mean)
{
	return pred_sync(ctx, PRED_MEAN, M, xq, mean, nullptr, nullptr);
}

extern "C" int gpemu_predict_mean_grad_enqueue(gpemu_ctx *ctx, int M, const double *xq) { return pred_enqueue(ctx, PRED_MEAN_GRAD, M, xq); }
extern "C" int gpemu_predict_mean_grad_collect(gpemu_ctx *ctx, int M, double *mean, double *grad) { return pred_collect(ctx, PRED_MEAN_GRAD, M, mean, nullptr, grad); }
extern "C" int gpemu_predict_mean_grad(gpemu_ctx *ctx, int M, const double *xq, double *mean, double *grad)
{
	return pred_sync(ctx, PRED_MEAN_GRAD, M, xq, mean, nullptr, grad);
}

extern "C" int gpemu_predict_var_grad_enqueue(gpemu_ctx *ctx, int M, const double *xq) { return pred_enqueue(ctx, PRED_VAR_GRAD, M, xq); }
extern "C" int gpemu_predict_var_grad_collect(gpemu_ctx *ctx, int M, double *mean, double *var, double *grad)
{
	return pred_collect(ctx, PRED_VAR_GRAD, M, mean, var, grad);
}
extern "C" int gpemu_predict_var_grad(gpemu_ctx *ctx, int M, const double *xq, double *mean, double *var, double *grad)
{
	return pred_sync(ctx, PRED_VAR_GRAD, M, xq, mean, var, grad);
}

// ---------------------------------------------------------------------------
// joint posterior covariance between the M query points of one call (gpemu.h):
//   Sigma_pq = c(x*_p, x*_q) - u_p . u_q + r_p^T Q r_q,   u = L^-1 k,  r = h(x*) - W^T k.
// ONE block of up to PRED_BATCH_MAX queries.  The k-vectors, V = Kq LinvAug^T (K never split: the u rows must be whole), the
// finish and Q r per query as in gpemu_predict_var_grad_dev, r kept beside; then the prior tiles c + r . (Q r) on the lower
// triangle of Sigma, the symmetric product Sigma -= U U^T on the GEMM of the factorisation's trailing update (tri, alpha = -1,
// beta = 1, A = B = dV, k over the Np columns of u) and the mirror.  The product works on Sigma in place with ldc = M: the GEMM
// moves C by single elements, so an odd M needs no padded scratch (its A and B rows are rows of dV, whose leading dimension
// Np + Rp is a multiple of 64).  Uses dKq, dV and its own dCovR; everything only enqueued on the context's stream.
// ---------------------------------------------------------------------------
// the part gpemu_predict_cov_dev and gpemu_predict_joint_factor_dev share: the lower 64 x 64 tiles of Sigma into S (M x M, leading
// dimension lds >= M), everything but the mirror.  The arguments have been checked.
static int predict_cov_lower(gpemu_ctx *ctx, int M, const double *xq_dev, double *mean_dev, double *cov_dev, long lds)
{
	const int Np = ctx->Np, Rp = ctx->Rp, d = ctx->d;
	const int mbp = round_up(M, 64);
	int rc = ensure_pred_batch(ctx, mbp);
	if (!rc) rc = grow(ctx, ctx->dCovR, (size_t)mbp * Rp + 2 * (size_t)mbp);
	if (rc) return rc;
	double *rkeep = ctx->dCovR, *spare = rkeep + (size_t)mbp * Rp;
	const long ldv = (long)Np + Rp;
	const CovParams &p = ctx->pred_cov;
	{
		ProfScope ps(ctx, GPEMU_PROF_FILL, 0.0, 8.0 * (double)mbp * Np);
		HIPCHK(ctx, fill_kvectors(ctx, ctx->dKq, xq_dev, M, mbp, p));
	}
	HIPCHK(ctx, launch_aug_product(ctx, aug_product_args(ctx, M)));
	HIPCHK(ctx, launch_predict_finish(ctx->stream, ctx->dV, ldv, M, Np, ctx->nreg, ctx->order, d, xq_dev, ctx->dBetaQ, ctx->kappa,
	                                  mean_dev ? mean_dev : spare, spare + mbp, 1, (long)mbp * ldv));
	HIPCHK(ctx, launch_predict_qr(ctx->stream, ctx->dV, ldv, M, Np, Rp, ctx->nreg, d, xq_dev, ctx->dBetaQ, rkeep));
	if (prof_on(ctx, GPEMU_PROF_COV)) ctx->prof.tag.push_back("predict_cov_prior");
	{
		// flops: per element of the lower triangle the squared distance (3 d) and the regression sum (2 nreg); bytes: the lower
		// triangle written once here (and mirrored once by gpemu_predict_cov_dev)
		ProfScope ps(ctx, GPEMU_PROF_COV, 0.5 * M * (double)M * (3.0 * d + 2.0 * ctx->nreg), 4.0 * M * (double)M);
		HIPCHK(ctx, launch_predict_cov_prior(ctx->stream, cov_dev, lds, xq_dev, M, d, p, rkeep, Rp, ctx->dV, ldv, Np, ctx->nreg));
	}
	GemmArgs g{};
	g.C = cov_dev; g.ldc = lds;
	g.A = ctx->dV; g.lda = ldv;
	g.B = ctx->dV; g.ldb = ldv;
	g.m = M; g.n = M; g.k0 = 0; g.k1 = Np; g.alpha = -1.0; g.beta = 1; g.tri = 1;
	HIPCHK(ctx, gemm(ctx, g));
	return GPEMU_OK;
}

extern "C" int gpemu_predict_cov_dev(gpemu_ctx *ctx, int M, const double *xq_dev, double *mean_dev, double *cov_dev)
{
	if (!ctx || M < 1 || M > PRED_BATCH_MAX || !xq_dev || !cov_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (const int rc = predict_cov_lower(ctx, M, xq_dev, mean_dev, cov_dev, M)) return rc;
	if (prof_on(ctx, GPEMU_PROF_COV)) ctx->prof.tag.push_back("predict_cov_mirror");
	{
		ProfScope ps(ctx, GPEMU_PROF_COV, 0.0, 4.0 * M * (double)M);
		HIPCHK(ctx, launch_predict_cov_mirror(ctx->stream, cov_dev, M, M));
	}
	return GPEMU_OK;
}

// host buffers: the queries go through the staging of the other host-buffer entries (hence not while one of their batches is
// pending), the result through dCov; every copy on the context's stream.  No enqueue / collect pair: the result is M^2 numbers.
extern "C" int gpemu_predict_cov(gpemu_ctx *ctx, int M, const double *xq, double *mean, double *cov)
{
	if (!ctx || M < 1 || M > PRED_BATCH_MAX || !xq || !cov) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->pred_pending.kind != PRED_NONE) return fail(ctx, GPEMU_ERR_STATE, "a prediction batch is enqueued: collect it first");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int d = ctx->d;
	int rc = ensure_pred_stage(ctx, M);
	if (!rc) rc = grow(ctx, ctx->dCov, (size_t)M * M, false, "out of device memory for the joint covariance (8 M^2 bytes)");
	if (rc) return rc;
	const size_t cap = ctx->stage_cap();
	double *hx = ctx->hStage, *hm = hx + cap * d;
	memcpy(hx, xq, (size_t)M * d * sizeof(double));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dXq, hx, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	rc = gpemu_predict_cov_dev(ctx, M, ctx->dXq, mean ? (double *)ctx->dMean : nullptr, ctx->dCov);
	if (rc) return rc;
	if (mean) HIPCHK(ctx, hipMemcpyAsync(hm, ctx->dMean, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(cov, ctx->dCov, (size_t)M * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if (mean) memcpy(mean, hm, (size_t)M * sizeof(double));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// hold-out validation and joint draws at the M query points of one call (gpemu.h): S = Sigma + diag(noise) is
// built in the factorisation's layout -- the lower tiles of predict_cov_lower straight into the tall matrix dJoint,
// (Mp + 64) x Mp with ld = Mp = M rounded up to 64; noise, identity pad and the rows yobs_a - mean in one staging pass --,
// factored in place by potrf_all through a view (plain launches: a single matrix of a size that changes from call to call),
// the solved rows turned into Mahalanobis distances and 2 sum log L_ii by the likelihood's Gram and finish kernels, and the
// factor cleaned into a plain lower triangle that stays resident for gpemu_predict_joint_draw.  Everything only enqueued on
// the context's stream; no atomics but the factorisation's info word.
// ---------------------------------------------------------------------------
constexpr int JOINT_DRAW_BLOCK = 1024;   // draws staged and multiplied at a time (8 * 1024 * Mp bytes of padded normals)

extern "C" int gpemu_predict_joint_factor_dev(gpemu_ctx *ctx, int M, const double *xq_dev, const double *noise_dev, int nobs,
                                              const double *yobs_dev, double *mean_dev, double *var_dev, double *werr_dev, double *stat_dev,
                                              int *info_dev)
{
	if (!ctx || M < 1 || M > PRED_BATCH_MAX || !xq_dev || !info_dev || nobs < 0 || nobs > JOINT_RHS || (nobs > 0 && !yobs_dev))
		return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	ctx->joint_M = 0;                    // the resident factor, if any, is about to be overwritten
	const int Mp = round_up(M, LEAF), Rp = JOINT_RHS;
	const size_t tall = ((size_t)Mp + Rp) * Mp;
	int rc = grow(ctx, ctx->dJoint, tall, false, "out of device memory for the joint factor (8 (M' + 64) M' bytes, M' = M rounded up to 64)");
	if (!rc) rc = grow(ctx, ctx->dJointMean, (size_t)Mp);
	if (!rc) rc = grow(ctx, ctx->dJointPart, (size_t)(Mp / LEAF + 1) * Rp * Rp + 2);
	if (rc) return rc;
	double *T = ctx->dJoint, *mu = ctx->dJointMean;
	double *part = ctx->dJointPart, *res = part + (size_t)(Mp / LEAF) * Rp * Rp;
	if ((rc = predict_cov_lower(ctx, M, xq_dev, mu, T, Mp))) return rc;
	if (prof_on(ctx, GPEMU_PROF_JOINT)) { ctx->prof.tag.push_back("joint_stage"); ctx->prof.tag.push_back("joint_clean"); }
	{
		// bytes: the 64 right-hand-side rows and the diagonal (the pad is at most 63 rows more)
		ProfScope ps(ctx, GPEMU_PROF_JOINT, 0.0, 8.0 * ((double)Rp * Mp + 2.0 * M));
		HIPCHK(ctx, launch_joint_stage(ctx->stream, T, Mp, M, noise_dev, mu, yobs_dev, nobs, var_dev));
	}
	HIPCHK(ctx, hipMemsetAsync(info_dev, 0x7f, sizeof(int), ctx->stream));     // INFO_NONE
	HIPCHK(ctx, trace_clear(ctx));
	{
		ProfScope ps(ctx, GPEMU_PROF_POTRF, (double)Mp * Mp * Mp / 3.0, 0.0);
		HIPCHK(ctx, potrf_all(ctx, Tall{T, info_dev, Mp, Rp, 1, (long)tall, 0}, 0));
	}
	if (stat_dev) {
		// G = Z Z^T of the solved rows Z_a = L_S^-1 (yobs_a - mean) and 2 sum_{p < M} log L_pp; stat = logdet, G_00, G_11, ...
		HIPCHK(ctx, launch_gram_partials(ctx->stream, T + (size_t)Mp * Mp, Mp, Mp, nobs, Rp, part));
		HIPCHK(ctx, launch_finish(ctx->stream, part, Mp / LEAF, Rp, nobs, T, Mp, M, res));
		HIPCHK(ctx, hipMemcpyAsync(stat_dev, res + (size_t)Rp * Rp, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
		if (nobs > 0)
			HIPCHK(ctx, hipMemcpy2DAsync(stat_dev + 1, sizeof(double), res, ((size_t)Rp + 1) * sizeof(double), sizeof(double), (size_t)nobs,
			                             hipMemcpyDeviceToDevice, ctx->stream));
	}
	if (werr_dev && nobs > 0)
		HIPCHK(ctx, hipMemcpy2DAsync(werr_dev, (size_t)M * sizeof(double), T + (size_t)Mp * Mp, (size_t)Mp * sizeof(double),
		                             (size_t)M * sizeof(double), (size_t)nobs, hipMemcpyDeviceToDevice, ctx->stream));
	if (mean_dev) HIPCHK(ctx, hipMemcpyAsync(mean_dev, mu, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
	{
		ProfScope ps(ctx, GPEMU_PROF_JOINT, 0.0, 4.0 * (double)Mp * Mp);
		HIPCHK(ctx, launch_joint_clean(ctx->stream, T, Mp, Mp));
	}
	ctx->joint_M = M;
	return GPEMU_OK;
}

// the device copies of a host call's arguments: one buffer, pieces at 16-byte multiples
struct JointIO { double *noise, *yobs, *var, *werr, *stat; };
static int joint_io(gpemu_ctx *ctx, int M, int nobs, JointIO *io)
{
	const size_t m2 = ((size_t)M + 1) & ~(size_t)1, ym = ((size_t)nobs * M + 1) & ~(size_t)1;
	if (const int rc = grow(ctx, ctx->dJointIO, 2 * m2 + 2 * ym + 2 + JOINT_RHS)) return rc;
	double *b = ctx->dJointIO;
	*io = JointIO{b, b + m2, b + m2 + ym, b + 2 * m2 + ym, b + 2 * m2 + 2 * ym};
	return GPEMU_OK;
}

// host buffers: the queries through the staging of the other host-buffer entries (hence not while one of their batches is
// pending), the other arguments through dJointIO.  The sign of noise is not looked at (the device-pointer entry cannot):
// a negative total on the diagonal shows up as a failed pivot.
extern "C" int gpemu_predict_joint_factor(gpemu_ctx *ctx, int M, const double *xq, const double *noise, int nobs, const double *yobs,
                                          double *mean, double *var, double *werr, double *maha, double *logdet, double *logpdf, int *info)
{
	if (!ctx || M < 1 || M > PRED_BATCH_MAX || !xq || !info || nobs < 0 || nobs > JOINT_RHS || (nobs > 0 && !yobs))
		return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->pred_pending.kind != PRED_NONE) return fail(ctx, GPEMU_ERR_STATE, "a prediction batch is enqueued: collect it first");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int d = ctx->d;
	JointIO io;
	int rc = ensure_pred_stage(ctx, M);
	if (!rc) rc = joint_io(ctx, M, nobs, &io);
	if (!rc) rc = grow(ctx, ctx->dJointInfo, 1);
	if (rc) return rc;
	double *hx = ctx->hStage;
	memcpy(hx, xq, (size_t)M * d * sizeof(double));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dXq, hx, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (noise) HIPCHK(ctx, hipMemcpyAsync(io.noise, noise, (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (nobs) HIPCHK(ctx, hipMemcpyAsync(io.yobs, yobs, (size_t)nobs * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	rc = gpemu_predict_joint_factor_dev(ctx, M, ctx->dXq, noise ? io.noise : nullptr, nobs, nobs ? io.yobs : nullptr, nullptr, io.var,
	                                    io.werr, io.stat, ctx->dJointInfo);
	if (rc) return rc;
	int word = 0;
	std::vector<double> stat((size_t)1 + nobs);
	HIPCHK(ctx, hipMemcpyAsync(&word, ctx->dJointInfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(stat.data(), io.stat, stat.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (mean) HIPCHK(ctx, hipMemcpyAsync(mean, ctx->dJointMean, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (var) HIPCHK(ctx, hipMemcpyAsync(var, io.var, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (werr && nobs) HIPCHK(ctx, hipMemcpyAsync(werr, io.werr, (size_t)nobs * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	const int bad = pivot_info(word);
	*info = bad;
	if (bad) {
		// mean and var were written before the factorisation began; everything behind it is undefined, and no factor is left
		ctx->joint_M = 0;
		if (werr) for (size_t i = 0; i < (size_t)nobs * M; i++) werr[i] = NAN;
		for (int a = 0; a < nobs; a++) { if (maha) maha[a] = NAN; if (logpdf) logpdf[a] = NAN; }
		if (logdet) *logdet = NAN;
		return fail(ctx, GPEMU_ERR_NOT_PD, "Sigma + diag(noise) is not positive definite");
	}
	if (logdet) *logdet = stat[0];
	for (int a = 0; a < nobs; a++) {
		if (maha) maha[a] = stat[1 + a];
		if (logpdf) logpdf[a] = -0.5 * (stat[1 + a] + stat[0] + M * 1.8378770664093454835606594728112);   // log 2 pi
	}
	return GPEMU_OK;
}

// out[s] = mean + L_S z[s]: per block of draws the staging pass and ONE product on the factorisation's GEMM, C = out (ldc = M),
// A = the padded normals, B = the resident factor, whose zeros above the diagonal let a tile stop at its last column (kend_mode)
extern "C" int gpemu_predict_joint_draw_dev(gpemu_ctx *ctx, int ndraw, const double *z_dev, double *out_dev)
{
	if (!ctx || ndraw < 1 || !z_dev || !out_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready || ctx->joint_M < 1) return fail(ctx, GPEMU_ERR_STATE, "no resident joint factor: call gpemu_predict_joint_factor first");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int M = ctx->joint_M, Mp = round_up(M, LEAF);
	if (const int rc = grow(ctx, ctx->dJointZ, (size_t)std::min(ndraw, JOINT_DRAW_BLOCK) * Mp)) return rc;
	for (int s0 = 0; s0 < ndraw; s0 += JOINT_DRAW_BLOCK) {
		const int nd = std::min(JOINT_DRAW_BLOCK, ndraw - s0);
		double *out = out_dev + (size_t)s0 * M;
		{
			if (prof_on(ctx, GPEMU_PROF_JOINT)) ctx->prof.tag.push_back("joint_draw_stage");
			ProfScope ps(ctx, GPEMU_PROF_JOINT, 0.0, 8.0 * nd * ((double)Mp + 2.0 * M));
			HIPCHK(ctx, launch_joint_draw_stage(ctx->stream, ctx->dJointZ, Mp, z_dev + (size_t)s0 * M, M, nd, out, ctx->dJointMean));
		}
		GemmArgs g{};
		g.C = out; g.ldc = M;
		g.A = ctx->dJointZ; g.lda = Mp;
		g.B = ctx->dJoint; g.ldb = Mp;
		g.m = nd; g.n = M; g.k0 = 0; g.k1 = Mp; g.alpha = 1.0; g.beta = 1; g.kend_mode = 1;
		HIPCHK(ctx, gemm(ctx, g));
	}
	return GPEMU_OK;
}

extern "C" int gpemu_predict_joint_draw(gpemu_ctx *ctx, int ndraw, const double *z, double *out)
{
	if (!ctx || ndraw < 1 || !z || !out) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready || ctx->joint_M < 1) return fail(ctx, GPEMU_ERR_STATE, "no resident joint factor: call gpemu_predict_joint_factor first");
	// (one rule for the host-buffer entries of the family, although the draws stage through a buffer of their own)
	if (ctx->pred_pending.kind != PRED_NONE) return fail(ctx, GPEMU_ERR_STATE, "a prediction batch is enqueued: collect it first");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int M = ctx->joint_M;
	const size_t blk = (size_t)std::min(ndraw, JOINT_DRAW_BLOCK) * M;
	// (dJointIO: a factor call's copies have been read by the time it returned)
	if (const int rc = grow(ctx, ctx->dJointIO, 2 * blk)) return rc;
	double *dz = ctx->dJointIO, *dout = dz + blk;
	for (int s0 = 0; s0 < ndraw; s0 += JOINT_DRAW_BLOCK) {
		const int nd = std::min(JOINT_DRAW_BLOCK, ndraw - s0);
		const size_t n = (size_t)nd * M;
		HIPCHK(ctx, hipMemcpyAsync(dz, z + (size_t)s0 * M, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		if (const int rc = gpemu_predict_joint_draw_dev(ctx, nd, dz, dout)) return rc;
		HIPCHK(ctx, hipMemcpyAsync(out + (size_t)s0 * M, dout, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	}
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// the resident factor and every buffer of the joint entries go back to the device (2.2 GB at M = 16384)
extern "C" int gpemu_predict_joint_release(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->joint_M = 0;
	for (auto *b : {&ctx->dJoint, &ctx->dJointMean, &ctx->dJointPart, &ctx->dJointZ, &ctx->dJointIO}) b->reset();
	ctx->dJointInfo.reset();
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// leave-one-out prediction at every training point (gpemu.h): one pass over the lower triangle of the resident L^-1 and a
// finishing launch, on the context's stream.  Touches only what the context owns (dLinvAug, dBetaQ, dY and its own
// scratch), so a context whose state came from gpemu_predict_setup_batch is served like any other.
// ---------------------------------------------------------------------------
extern "C" int gpemu_loo_dev(gpemu_ctx *ctx, double *mean_dev, double *var_dev)
{
	if (!ctx || !mean_dev || !var_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	const int N = ctx->N, Np = ctx->Np, nreg = ctx->nreg;
	if (N <= nreg + 1) return fail(ctx, GPEMU_ERR_ARG, "leave-one-out needs N > nregression_fns + 1");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int rc = grow(ctx, ctx->dLooPart, loo_scratch_elems(N, Np));
	if (rc) return rc;
	if (prof_on(ctx, GPEMU_PROF_LOO)) { ctx->prof.tag.push_back("loo_colsq"); ctx->prof.tag.push_back("loo_finish"); }
	{
		ProfScope ps(ctx, GPEMU_PROF_LOO, (double)N * (N + 1), 8.0 * ((double)N * (N + 1) / 2));
		HIPCHK(ctx, launch_loo_colsq(ctx->stream, ctx->dLinvAug, Np, N, Np, ctx->dLooPart));
	}
	{
		// the partials (lower half of the chunk x column table), gamma and the W^T rows, y in; mean and variance out
		ProfScope ps(ctx, GPEMU_PROF_LOO, 2.0 * N * nreg * nreg,
		             8.0 * ((double)loo_scratch_elems(N, Np) / 2 + (double)N * (nreg + 4)));
		HIPCHK(ctx, launch_loo_finish(ctx->stream, ctx->dLooPart, ctx->dLinvAug, Np, N, Np, nreg, ctx->dBetaQ, ctx->dY, mean_dev,
		                              var_dev));
	}
	return GPEMU_OK;
}

extern "C" int gpemu_loo(gpemu_ctx *ctx, double *mean, double *var)
{
	if (!ctx || !mean || !var) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	const size_t N = (size_t)ctx->N;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	int rc = grow(ctx, ctx->dLoo, 2 * N);
	if (!rc) rc = grow(ctx, ctx->hLoo, 2 * N);
	if (!rc) rc = gpemu_loo_dev(ctx, ctx->dLoo, ctx->dLoo + N);
	if (rc) return rc;
	HIPCHK(ctx, hipMemcpyAsync(ctx->hLoo, ctx->dLoo, 2 * N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	memcpy(mean, ctx->hLoo, N * sizeof(double));
	memcpy(var, ctx->hLoo + N, N * sizeof(double));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// K-fold / leave-group-out validation (gpemu.h): for every group B the joint leave-B-out prediction from the
// resident L^-1, gamma, W^T and Q.  Per chunk of groups: gather the members' columns of L^-1 as rows Z_g, (C^-1)_BB = Z_g Z_g^T
// (one batched product into the tall layout), staging (minus W_B Q W_B^T, pad, gamma_B, identity rows), ONE lock-step
// factorisation with inverse rows through a view of dLgoT, |w|^2 and sum log R_ii by the likelihood's Gram and finish kernels
// (one right-hand side, Rp = 1), the finishing pass.  Plain launches (the shape changes from call to call), everything on the
// context's stream, only buffers of its own.
// ---------------------------------------------------------------------------
constexpr double LGO_BUDGET = 2147483648.0;   // bytes of 8 nbc bp (Np + 2 bp + 64) a chunk may take: fixed, so the chunking depends on the call alone
constexpr int LGO_BP_MAX = 16384;

struct LgoPlan {
	int bp = 0, nbc = 0;
	std::vector<int> count;
};

// the model-dependent argument checks, nothing allocated or launched; the padded size and the chunk size
static int lgo_plan(gpemu_ctx *ctx, int ngroups, const int *group, LgoPlan *pl)
{
	const int N = ctx->N;
	if (ngroups > N) return fail(ctx, GPEMU_ERR_ARG, "leave-group-out: more groups than training points");
	pl->count.assign((size_t)ngroups, 0);
	for (int i = 0; i < N; i++) {
		if (group[i] < -1 || group[i] >= ngroups) return fail(ctx, GPEMU_ERR_ARG, "leave-group-out: a label outside -1 .. ngroups-1");
		if (group[i] >= 0) pl->count[group[i]]++;
	}
	int bmax = 0;
	for (int g = 0; g < ngroups; g++) {
		if (!pl->count[g]) return fail(ctx, GPEMU_ERR_ARG, "leave-group-out: a label without members");
		bmax = std::max(bmax, pl->count[g]);
	}
	if (N - bmax <= ctx->nreg) return fail(ctx, GPEMU_ERR_ARG, "leave-group-out needs N - (largest group) > nregression_fns");
	if (round_up(bmax, LEAF) > LGO_BP_MAX) return fail(ctx, GPEMU_ERR_ARG, "leave-group-out: a group of more than 16384 points");
	pl->bp = round_up(bmax, LEAF);
	const double per = 8.0 * pl->bp * ((double)ctx->Np + 2.0 * pl->bp + LEAF);
	pl->nbc = std::max(1, std::min(std::min(ngroups, GPEMU_MAX_BATCH), (int)(LGO_BUDGET / per)));
	return GPEMU_OK;
}

// What follows the staging launch for one chunk of nbc staged tall matrices T (tstride apart, padded to bp): the info words to
// INFO_NONE, ONE lock-step factorisation with inverse rows, |w|^2 and sum log R_ii by the likelihood's Gram and finish kernels
// (one right-hand side, Rp = 1), the finishing pass.  info: nbc words, part: nbc * (bp / 64 + 2) doubles.  lgo_run calls it per
// chunk on the context's buffers, gpemu_test_resident_launch (GPEMU_RES_LGO_TAIL) on buffers of its own.
static int lgo_chunk_tail(gpemu_ctx *ctx, double *T, long tstride, int nbc, int bp, int *info, double *part, const int *d_members,
                          const int *d_moff, const int *d_bsize, const double *dY, int g0, int ngroups, double *mean_dev, double *var_dev,
                          double *werr_dev, double *stat_dev, int *info_dev)
{
	double *res = part + (size_t)nbc * (bp / LEAF);
	HIPCHK(ctx, hipMemsetAsync(info, 0x7f, (size_t)nbc * sizeof(int), ctx->stream));     // INFO_NONE
	HIPCHK(ctx, trace_clear(ctx));
	{
		ProfScope ps(ctx, GPEMU_PROF_POTRF, (double)nbc * bp * bp * bp / 3.0, 0.0);
		HIPCHK(ctx, potrf_all(ctx, Tall{T, info, bp, LEAF, nbc, tstride, 0}, 1));
	}
	// |w|^2 of the solved right-hand-side row and 2 sum log R_ii (the pad's pivots are 1) per group
	HIPCHK(ctx, launch_gram_partials(ctx->stream, T + (size_t)bp * bp, bp, bp, 1, 1, part, nbc, tstride));
	HIPCHK(ctx, launch_finish(ctx->stream, part, bp / LEAF, 1, 1, T, bp, bp, res, nbc, tstride, 2));
	{
		ProfScope ps(ctx, GPEMU_PROF_LGO, 0.0, 8.0 * nbc * bp * (bp / 2.0 + 4.0));
		HIPCHK(ctx, launch_lgo_finish(ctx->stream, T, tstride, nbc, bp, d_members, d_moff, d_bsize, info, res, dY, g0, ngroups, mean_dev,
		                              var_dev, werr_dev, stat_dev, info_dev));
	}
	return GPEMU_OK;
}

// the status of a leave-group-out call from the decoded info words of its groups
static int lgo_status(gpemu_ctx *ctx, int ngroups, const int *info)
{
	for (int g = 0; g < ngroups; g++)
		if (info[g]) return fail(ctx, GPEMU_ERR_NOT_PD, "leave-group-out: P_BB of a group is not positive definite");
	return GPEMU_OK;
}

static int lgo_run(gpemu_ctx *ctx, const LgoPlan &pl, int ngroups, const int *group, double *mean_dev, double *var_dev, double *werr_dev,
                   double *stat_dev, int *info_dev)
{
	const int N = ctx->N, Np = ctx->Np, bp = pl.bp, nbc_max = pl.nbc;
	const size_t tstride = ((size_t)2 * bp + LEAF) * bp, ntab = 2 * (size_t)N + 2 * (size_t)ngroups;
	const char *oom = "out of device memory for leave-group-out (8 nbc bp (Np + 2 bp + 64) bytes per chunk of nbc groups padded to bp)";
	int rc = grow(ctx, ctx->dLgoZ, (size_t)nbc_max * bp * Np, false, oom);
	if (!rc) rc = grow(ctx, ctx->dLgoT, (size_t)nbc_max * tstride, false, oom);
	if (!rc) rc = grow(ctx, ctx->dLgoPart, (size_t)nbc_max * (bp / LEAF + 2));
	if (!rc) rc = grow(ctx, ctx->dLgoInfo, (size_t)nbc_max);
	if (!rc) rc = grow(ctx, ctx->dLgoTab, ntab);
	if (!rc) rc = grow(ctx, ctx->hLgoTab, ntab);
	if (rc) return rc;
	if (!ctx->lgo_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->lgo_ev, hipEventDisableTiming));
	HIPCHK(ctx, hipEventSynchronize(ctx->lgo_ev));        // the previous call's upload has left the pinned tables (a never-recorded event is complete)
	// tables: colrow[N], members[N] (group after group, ascending design index), moff[ngroups], bsize[ngroups]
	int *colrow = ctx->hLgoTab, *members = colrow + N, *moff = members + N, *bsize = moff + ngroups;
	for (int g = 0, o = 0; g < ngroups; g++) { moff[g] = o; o += pl.count[g]; bsize[g] = 0; }
	for (int i = 0; i < N; i++) {
		const int g = group[i];
		colrow[i] = -1;
		if (g < 0) continue;
		colrow[i] = g * bp + bsize[g];
		members[moff[g] + bsize[g]++] = i;
	}
	for (int i = moff[ngroups - 1] + bsize[ngroups - 1]; i < N; i++) members[i] = 0;   // (behind the last member: uploaded, never read)
	HIPCHK(ctx, hipMemcpyAsync(ctx->dLgoTab, ctx->hLgoTab, ntab * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipEventRecord(ctx->lgo_ev, ctx->stream));
	const int *d_colrow = ctx->dLgoTab, *d_members = d_colrow + N, *d_moff = d_members + N, *d_bsize = d_moff + ngroups;
	// NaN (all bits set) for the points that are never left out; every member's element is overwritten below
	HIPCHK(ctx, hipMemsetAsync(mean_dev, 0xff, (size_t)N * sizeof(double), ctx->stream));
	HIPCHK(ctx, hipMemsetAsync(var_dev, 0xff, (size_t)N * sizeof(double), ctx->stream));
	if (werr_dev) HIPCHK(ctx, hipMemsetAsync(werr_dev, 0xff, (size_t)N * sizeof(double), ctx->stream));
	double *Z = ctx->dLgoZ, *T = ctx->dLgoT, *part = ctx->dLgoPart;
	for (int g0 = 0; g0 < ngroups; g0 += nbc_max) {
		const int nbc = std::min(nbc_max, ngroups - g0);
		if (prof_on(ctx, GPEMU_PROF_LGO)) for (const char *t : {"lgo_gather", "lgo_stage", "lgo_finish"}) ctx->prof.tag.push_back(t);
		{
			ProfScope ps(ctx, GPEMU_PROF_LGO, 0.0, 8.0 * nbc * bp * (double)Np);
			HIPCHK(ctx, launch_lgo_gather(ctx->stream, ctx->dLinvAug, Np, N, Np, d_colrow, d_bsize, g0, nbc, bp, Z));
		}
		GemmArgs g{};
		g.C = T; g.ldc = bp;
		g.A = Z; g.lda = Np;
		g.B = Z; g.ldb = Np;
		g.m = bp; g.n = bp; g.k0 = 0; g.k1 = Np; g.alpha = 1.0; g.beta = 0;
		g.tri = 1; g.diag_off = 0;
		g.nbatch = nbc; g.bsC = (long)tstride; g.bsA = g.bsB = (long)bp * Np;
		HIPCHK(ctx, gemm(ctx, g));
		{
			ProfScope ps(ctx, GPEMU_PROF_LGO, 0.0, 8.0 * nbc * bp * (2.0 * bp + LEAF));
			HIPCHK(ctx, launch_lgo_stage(ctx->stream, T, (long)tstride, g0, nbc, bp, d_members, d_moff, d_bsize, ctx->dLinvAug, Np, Np,
			                             ctx->nreg, ctx->dBetaQ));
		}
		if (const int rc2 = lgo_chunk_tail(ctx, T, (long)tstride, nbc, bp, ctx->dLgoInfo, part, d_members, d_moff, d_bsize, ctx->dY, g0, ngroups,
		                                   mean_dev, var_dev, werr_dev, stat_dev, info_dev))
			return rc2;
	}
	return GPEMU_OK;
}

extern "C" int gpemu_lgo_dev(gpemu_ctx *ctx, int ngroups, const int *group, double *mean_dev, double *var_dev, double *werr_dev,
                             double *stat_dev, int *info_dev)
{
	if (!ctx || ngroups < 1 || !group || !mean_dev || !var_dev || !info_dev) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	LgoPlan pl;
	if (const int rc = lgo_plan(ctx, ngroups, group, &pl)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	return lgo_run(ctx, pl, ngroups, group, mean_dev, var_dev, werr_dev, stat_dev, info_dev);
}

extern "C" int gpemu_lgo(gpemu_ctx *ctx, int ngroups, const int *group, double *mean, double *var, double *werr, double *maha,
                         double *logdet, double *logpdf, int *info)
{
	if (!ctx || ngroups < 1 || !group || !mean || !var || !info) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	LgoPlan pl;
	if (const int rc0 = lgo_plan(ctx, ngroups, group, &pl)) return rc0;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t N = (size_t)ctx->N, G = (size_t)ngroups;
	int rc = grow(ctx, ctx->dLgoOut, 3 * N + 3 * G);
	if (!rc) rc = grow(ctx, ctx->dLgoInfoOut, G);
	if (rc) return rc;
	double *o = ctx->dLgoOut, *st = o + 3 * N;
	rc = lgo_run(ctx, pl, ngroups, group, o, o + N, o + 2 * N, st, ctx->dLgoInfoOut);
	if (rc) return rc;
	HIPCHK(ctx, hipMemcpyAsync(mean, o, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(var, o + N, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (werr) HIPCHK(ctx, hipMemcpyAsync(werr, o + 2 * N, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (maha) HIPCHK(ctx, hipMemcpyAsync(maha, st, G * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (logdet) HIPCHK(ctx, hipMemcpyAsync(logdet, st + G, G * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (logpdf) HIPCHK(ctx, hipMemcpyAsync(logpdf, st + 2 * G, G * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(info, ctx->dLgoInfoOut, G * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return lgo_status(ctx, ngroups, info);
}

// every buffer of the leave-group-out entries goes back to the device
extern "C" int gpemu_lgo_release(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	for (auto *b : {&ctx->dLgoZ, &ctx->dLgoT, &ctx->dLgoPart, &ctx->dLgoOut}) b->reset();
	for (auto *b : {&ctx->dLgoTab, &ctx->dLgoInfo, &ctx->dLgoInfoOut}) b->reset();
	ctx->hLgoTab.reset();
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// main effects and Sobol indices of the posterior mean in closed form (gpemu.h): three launches on a's
// stream -- the per-point integrals of both contexts, the N x N sweep of pair terms into per-tile partials, the finish.
// Reads dX, dBetaQ and the gamma row of dLinvAug of both contexts; everything it writes is its own (dSens*), all in a.
// ---------------------------------------------------------------------------
// every check of a call, nothing allocated or launched; fills the box with both contexts' squared inverse lengths
static int sens_check(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi, SensBox *bx)
{
	if (!a->pred_ready || !b->pred_ready) return fail(a, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (a->kind != GPEMU_POWEREXP || b->kind != GPEMU_POWEREXP)
		return fail(a, GPEMU_ERR_ARG, "sensitivity: the closed form exists for the power-exponential covariance only (a Matern kernel is no product over the coordinates)");
	if (a->device != b->device) return fail(a, GPEMU_ERR_ARG, "sensitivity: the two contexts are on different devices");
	if (a->N != b->N || a->d != b->d || (a != b && a->hX != b->hX))
		return fail(a, GPEMU_ERR_ARG, "sensitivity: the two contexts hold different designs");
	if (a->order != b->order) return fail(a, GPEMU_ERR_ARG, "sensitivity: the two contexts differ in their regression order");
	const int d = a->d;
	int ngauss = 0;
	for (int l = 0; l < d; l++) {
		if (a->sens_kind[l] != b->sens_kind[l]) return fail(a, GPEMU_ERR_ARG, "sensitivity: the two contexts differ in their input measure");
		if (a->sens_kind[l] == GPEMU_MEASURE_GAUSS) {
			// lo: the mean, hi: the standard deviation
			if (!std::isfinite(lo[l]) || !std::isfinite(hi[l]) || !(hi[l] > 0.0))
				return fail(a, GPEMU_ERR_ARG, "sensitivity: a Gaussian coordinate needs a finite mean and a finite standard deviation > 0");
			ngauss++;
		} else if (!std::isfinite(lo[l]) || !std::isfinite(hi[l]) || !(hi[l] > lo[l]) || !std::isfinite(hi[l] - lo[l]))
			return fail(a, GPEMU_ERR_ARG, "sensitivity: every bound must be finite, with hi > lo");
	}
	memset(bx, 0, sizeof *bx);
	bx->d = d;
	bx->meas = ngauss == 0 ? 0 : (ngauss == d ? 1 : 2);
	for (int l = 0; l < d; l++) {
		bx->kind[l] = a->sens_kind[l];
		bx->s[l] = 2.0 * a->pred_cov.w[l] * a->pred_cov.w[l];      // w = sqrt(1/2) e^-theta: s = e^(-2 theta)
		bx->t[l] = 2.0 * b->pred_cov.w[l] * b->pred_cov.w[l];
		bx->lo[l] = lo[l];
		bx->hi[l] = hi[l];
	}
	return GPEMU_OK;
}

// flops of the pair factors of one pair of points (the rule at GPEMU_PROF_SENS*): a uniform coordinate's is one exp and two
// erf / erfc among 16 flops, 19; a Gaussian one's is one exp among 11, 12.  ncoord: how many factors the pair evaluates (d in
// the sweep of gpemu_sens_cov; the blocks' 8 and 16 in the pair sweep), taken in the kinds' proportion
static double sens_pair_flops(const SensBox &bx, double ncoord)
{
	int ng = 0;
	for (int l = 0; l < bx.d; l++) ng += bx.kind[l] == GPEMU_MEASURE_GAUSS;
	return ncoord * (19.0 * (bx.d - ng) + 12.0 * ng) / bx.d;
}

extern "C" int gpemu_sens_set_measure(gpemu_ctx *ctx, const int *kind)
{
	if (!ctx) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	for (int l = 0; kind && l < ctx->d; l++)
		if (kind[l] != GPEMU_MEASURE_UNIFORM && kind[l] != GPEMU_MEASURE_GAUSS)
			return fail(ctx, GPEMU_ERR_ARG, "sensitivity: a measure kind is GPEMU_MEASURE_UNIFORM or GPEMU_MEASURE_GAUSS");
	for (int l = 0; l < ctx->d; l++) ctx->sens_kind[l] = kind ? kind[l] : GPEMU_MEASURE_UNIFORM;
	return GPEMU_OK;
}

extern "C" int gpemu_sens_get_measure(const gpemu_ctx *ctx, int *kind)
{
	if (!ctx || !kind) return GPEMU_ERR_ARG;
	if (!ctx->dX) return GPEMU_ERR_STATE;
	std::copy(ctx->sens_kind, ctx->sens_kind + ctx->d, kind);
	return GPEMU_OK;
}

// a's stream behind b's pending work, without the host waiting
static int sens_order_streams(gpemu_ctx *a, gpemu_ctx *b)
{
	if (a == b) return GPEMU_OK;
	if (!a->sens_ev) HIPCHK(a, hipEventCreateWithFlags(&a->sens_ev, hipEventDisableTiming));
	if (!a->sens_ev2) HIPCHK(a, hipEventCreateWithFlags(&a->sens_ev2, hipEventDisableTiming));
	HIPCHK(a, hipEventRecord(a->sens_ev, b->stream));
	HIPCHK(a, hipStreamWaitEvent(a->stream, a->sens_ev, 0));
	return GPEMU_OK;
}

static int sens_prep(gpemu_ctx *a, const SensBox &bx, int cls = GPEMU_PROF_SENS)
{
	const int N = a->N, d = a->d;
	int rc = grow(a, a->dSensPrep, sens_prep_elems(N, d));
	if (!rc) rc = grow(a, a->dSensCst, (size_t)SENS_CST_ROWS * GPEMU_MAX_PARAMS);
	if (rc) return rc;
	// per point and coordinate of either context two erf and two exp with some forty flops around them; the tables out
	ProfScope ps(a, cls, 2.0 * N * d * 44.0, 8.0 * ((double)sens_prep_elems(N, d) + (double)N * d));
	HIPCHK(a, launch_sens_prep(a->stream, a->dX, N, bx, a->dSensPrep, a->dSensCst));
	return GPEMU_OK;
}

extern "C" int gpemu_sens_cov_dev(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi, double *out_dev)
{
	if (!a || !b || !lo || !hi || !out_dev) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_check(a, b, lo, hi, &bx)) return rc;
	HIPCHK(a, hipSetDevice(a->device));
	const int N = a->N, d = a->d, Np = a->Np;
	if (const int rc = grow(a, a->dSensPart, sens_part_elems(N, d))) return rc;
	if (const int rc = sens_order_streams(a, b)) return rc;
	if (prof_on(a, GPEMU_PROF_SENS)) for (const char *t : {"sens_prep", "sens_sweep", "sens_finish"}) a->prof.tag.push_back(t);
	if (const int rc = sens_prep(a, bx)) return rc;
	const double *gamA = a->dLinvAug + (size_t)Np * Np, *gamB = b->dLinvAug + (size_t)Np * Np;
	{
		// per pair and coordinate: one exp and two erf / erfc (counted as one flop each) among 16 flops, then 2 (2 d + 1) for the sums
		ProfScope ps(a, GPEMU_PROF_SENS, (double)N * N * (sens_pair_flops(bx, d) + 2.0), 8.0 * (double)sens_part_elems(N, d));
		HIPCHK(a, launch_sens_sweep(a->stream, a->dX, N, d, gamA, gamB, a->dSensPrep, a->dSensCst, bx.meas, a->dSensPart));
	}
	{
		ProfScope ps(a, GPEMU_PROF_SENS, (double)sens_part_elems(N, d), 8.0 * (double)sens_part_elems(N, d));
		HIPCHK(a, launch_sens_finish(a->stream, a->dSensPart, N, d, a->order, gamA, a->dBetaQ, a->pred_cov.amp, gamB, b->dBetaQ,
		                             b->pred_cov.amp, a->dSensPrep, a->dSensCst, out_dev));
	}
	if (a != b) {
		// b's later work (a new set-up would rewrite its gamma) runs behind this call
		HIPCHK(a, hipEventRecord(a->sens_ev2, a->stream));
		HIPCHK(a, hipStreamWaitEvent(b->stream, a->sens_ev2, 0));
	}
	return GPEMU_OK;
}

extern "C" int gpemu_sens_cov(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi, double *e0, double *cov_all,
                              double *cov_first, double *cov_rest)
{
	if (!a || !b || !lo || !hi || !e0 || !cov_all || !cov_first || !cov_rest) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_check(a, b, lo, hi, &bx)) return rc;
	HIPCHK(a, hipSetDevice(a->device));
	const size_t d = (size_t)a->d;
	if (const int rc = grow(a, a->dSensOut, 3 + 2 * (size_t)GPEMU_MAX_PARAMS)) return rc;
	if (const int rc = gpemu_sens_cov_dev(a, b, lo, hi, a->dSensOut)) return rc;
	std::vector<double> o(3 + 2 * d);
	HIPCHK(a, hipMemcpyAsync(o.data(), a->dSensOut, o.size() * sizeof(double), hipMemcpyDeviceToHost, a->stream));
	HIPCHK(a, hipStreamSynchronize(a->stream));
	e0[0] = o[0];
	e0[1] = o[1];
	*cov_all = o[2];
	memcpy(cov_first, o.data() + 3, d * sizeof(double));
	memcpy(cov_rest, o.data() + 3 + d, d * sizeof(double));
	return GPEMU_OK;
}

extern "C" int gpemu_sens_main(gpemu_ctx *ctx, const double *lo, const double *hi, int ngrid, const double *grid, double *e0, double *main)
{
	if (!ctx || !lo || !hi || !grid || !e0 || !main || ngrid < 1) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_check(ctx, ctx, lo, hi, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int N = ctx->N, d = ctx->d, Np = ctx->Np;
	const size_t ng = (size_t)d * ngrid;
	int rc = grow(ctx, ctx->dSensGrid, 2 * ng);
	if (!rc) rc = grow(ctx, ctx->dSensOut, 3 + 2 * (size_t)GPEMU_MAX_PARAMS);
	if (rc) return rc;
	HIPCHK(ctx, hipMemcpyAsync(ctx->dSensGrid, grid, ng * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (prof_on(ctx, GPEMU_PROF_SENS)) for (const char *t : {"sens_prep", "sens_main"}) ctx->prof.tag.push_back(t);
	if ((rc = sens_prep(ctx, bx))) return rc;
	{
		ProfScope ps(ctx, GPEMU_PROF_SENS, (double)ng * N * 6.0, 8.0 * 2.0 * (double)ng);
		HIPCHK(ctx, launch_sens_main(ctx->stream, ctx->dX, N, d, ctx->order, ctx->dLinvAug + (size_t)Np * Np, ctx->dBetaQ, ctx->pred_cov.amp,
		                             ctx->dSensPrep, ctx->dSensCst, ctx->dSensGrid, ngrid, ctx->dSensOut, ctx->dSensGrid + ng));
	}
	HIPCHK(ctx, hipMemcpyAsync(main, ctx->dSensGrid + ng, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(e0, ctx->dSensOut, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// every buffer of the sensitivity entries goes back to the device
extern "C" int gpemu_sens_release(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	for (auto *b : {&ctx->dSensPrep, &ctx->dSensCst, &ctx->dSensPart, &ctx->dSensOut, &ctx->dSensGrid, &ctx->dSensP, &ctx->dSensG,
	                &ctx->dSensPostPart, &ctx->dSensPex2, &ctx->dSensPairPart, &ctx->dSensPairOut})
		b->reset();
	ctx->sens_post_N = 0;
	for (auto *b : {&ctx->dDesignKH, &ctx->dDesignHm, &ctx->dDesignPrepQ, &ctx->dDesignA, &ctx->dDesignT, &ctx->dDesignR, &ctx->dDesignB,
	                &ctx->dDesignPart, &ctx->dDesignOut})
		b->reset();
	ctx->design_serial = 0;
	ctx->design_mb = 0;
	for (auto *b : {&ctx->dBatchW, &ctx->dBatchLam, &ctx->dBatchMu, &ctx->dBatchE, &ctx->dBatchSv, &ctx->dBatchDots, &ctx->dBatchSt, &ctx->dBatchTab,
	                &ctx->dBatchIO})
		b->reset();
	ctx->batch_mb = ctx->batch_nb = 0;
	return GPEMU_OK;
}

// beta and gamma = C^-1 (y - H beta) exactly as the prediction state holds them (parity tests: a reference that is to be
// met to rounding must start from the same two vectors, not from another factorisation's)
extern "C" int gpemu_test_pred_state(gpemu_ctx *ctx, double *beta, double *gamma)
{
	if (!ctx || !beta || !gamma) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipMemcpyAsync(beta, ctx->dBetaQ, (size_t)ctx->nreg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(gamma, ctx->dLinvAug + (size_t)ctx->Np * ctx->Np, (size_t)ctx->N * sizeof(double), hipMemcpyDeviceToHost,
	                           ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// explicit inverse: S = Aug Aug^T with Aug = [Z^T ; U]  ->  S[Rp+i][Rp+j] = (C^-1)_ij,
// S[Rp+i][a] = (C^-1 [y|H])_ia   (lower triangle only)
// ---------------------------------------------------------------------------
// corners of the nbc elements b0 .. b0+nbc-1 of the factored batch t (one batched product) into S: squares of side and
// leading dimension lds = Np + Rp, one after the other
static hipError_t build_corner(gpemu_ctx *ctx, const Tall &t, double *S, long lds, int b0 = 0, int nbc = 1)
{
	GemmArgs g{};
	g.C = S; g.ldc = lds;
	g.A = t.T + (size_t)b0 * t.stride + (size_t)t.Np * t.Np; g.lda = t.Np;
	g.B = g.A; g.ldb = t.Np;
	g.m = (int)lds; g.n = (int)lds; g.k0 = 0; g.k1 = t.Np; g.alpha = 1.0; g.beta = 0;
	g.tri = 1; g.diag_off = 0;
	g.kstart_mode = 1; g.kstart_off = t.Rp;
	g.nbatch = nbc; g.bsC = lds * lds; g.bsA = g.bsB = t.stride;
	return gemm(ctx, g);
}

// the corner of a context with a prediction set-up, in dS (side and leading dimension S_dim), built once per set-up
// (gpemu_get_cinverse and gpemu_sens_post)
static int ensure_corner(gpemu_ctx *ctx)
{
	if (!ctx->cinv_ready && !ctx->fact_in_T) {
		// set up by gpemu_predict_setup_batch as a later component: its factorisation ran in the first context's workspace
		// (round 5: reading this context's own, never allocated workspace here was a GPU memory fault).  The explicit inverse is
		// the slow path anyway (N x N doubles to the host): factor this component alone, same thetas, same bits, into this
		// context's workspace -- and nothing else.  The prediction state a whole set-up would rebuild from it is the one already
		// here bit for bit, so it stays, and with it what belongs to the set-up: the joint factor, the transposed copy, pred_serial
		// (the design block and the target store).  Not gpemu_predict_setup: its invalidate_prediction dropped all of those.
		const std::vector<double> th = ctx->last_thetas;
		CovParams p;
		int info = 0;
		int rc = factor_with_inverse(ctx, th.data(), (int)th.size(), &p, &info);
		if (rc) return rc;
		ctx->fact_in_T = true;
	}
	if (!ctx->cinv_ready) {
		const size_t dim = (size_t)ctx->Np + ctx->Rp;
		int rc = grow(ctx, ctx->dS, dim * dim);
		if (rc) return rc;
		ctx->S_dim = dim;
		HIPCHK(ctx, build_corner(ctx, tall_of(ctx), ctx->dS, (long)dim));
		ctx->cinv_ready = true;
	}
	return GPEMU_OK;
}

extern "C" int gpemu_get_cinverse(gpemu_ctx *ctx, double *cinv_out)
{
	if (!ctx || !cinv_out) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (const int rc = ensure_corner(ctx)) return rc;
	const int N = ctx->N, Rp = ctx->Rp;
	const size_t dim = ctx->S_dim;
	HIPCHK(ctx, hipMemcpy2DAsync(cinv_out, (size_t)N * sizeof(double), ctx->dS + (size_t)Rp * dim + Rp,
	                             dim * sizeof(double), (size_t)N * sizeof(double), N, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	// mirror the lower triangle into the upper one, 64 x 64 blocks at a time (a plain column walk over 512 MB at N = 8192
	// misses the cache on every element: 0.3 s of alloc_emulator_struct's 0.4)
	for (int i0 = 0; i0 < N; i0 += 64)
		for (int j0 = i0; j0 < N; j0 += 64)
			for (int i = i0; i < std::min(i0 + 64, N); i++)
				for (int j = std::max(j0, i + 1); j < std::min(j0 + 64, N); j++) cinv_out[(size_t)i * N + j] = cinv_out[(size_t)j * N + i];
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// emulator uncertainty of the main effects and Sobol indices (gpemu.h).  gpemu_sens_post: prep, the corner
// C^-1 = U U^T (built once per set-up, shared with gpemu_get_cinverse, read only), P and G from it, the weighted sweep over
// the lower tiles, the finish.  Writes dSensPrep, dSensCst and its own dSensP, dSensG, dSensPostPart.
// ---------------------------------------------------------------------------
extern "C" int gpemu_sens_post_dev(gpemu_ctx *ctx, const double *lo, const double *hi, double *out_dev)
{
	if (!ctx || !lo || !hi || !out_dev) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_check(ctx, ctx, lo, hi, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int N = ctx->N, d = ctx->d, nreg = ctx->nreg, Rp = ctx->Rp;
	const size_t ldp = (size_t)round_up(N, 64), npart = sens_post_part_elems(N, d);
	const double ntl = (double)(ldp / 64) * (double)(ldp / 64 + 1) / 2.0;           // lower tiles
	int rc = grow(ctx, ctx->dSensPostPart, npart);
	if (!rc) rc = grow(ctx, ctx->dSensP, ldp * ldp);
	if (!rc) rc = grow(ctx, ctx->dSensG, (size_t)N * nreg);
	if (rc) return rc;
	if (prof_on(ctx, GPEMU_PROF_SENS_POST))
		for (const char *t : {"sens_prep", "sens_pmat", "sens_sweep_weighted", "sens_post_finish"}) ctx->prof.tag.push_back(t);
	if ((rc = sens_prep(ctx, bx, GPEMU_PROF_SENS_POST))) return rc;
	if ((rc = ensure_corner(ctx))) return rc;
	const double *Q = ctx->dBetaQ + nreg;
	{
		// per tile: G for its 64 rows (2 nreg^2 each), then 2 nreg + 1 per pair; the corner's tile read, P's written
		ProfScope ps(ctx, GPEMU_PROF_SENS_POST, ntl * (128.0 * nreg * nreg + 4096.0 * (2.0 * nreg + 1.0)), 8.0 * ntl * 8192.0);
		HIPCHK(ctx, launch_sens_pmat(ctx->stream, ctx->dS, (long)ctx->S_dim, Rp, Q, N, nreg, ctx->dSensG, ctx->dSensP));
	}
	{
		// the pair terms of GPEMU_PROF_SENS with one product more per coordinate and the rank-one sum; P read, the sums written
		ProfScope ps(ctx, GPEMU_PROF_SENS_POST, ntl * 4096.0 * (sens_pair_flops(bx, d) + d + 3.0), 8.0 * (ntl * 4096.0 + (double)npart));
		HIPCHK(ctx, launch_sens_sweep_weighted(ctx->stream, ctx->dX, N, d, ctx->dSensPrep, ctx->dSensCst, bx.meas, ctx->dSensP,
		                                       ctx->dSensPostPart));
	}
	{
		ProfScope ps(ctx, GPEMU_PROF_SENS_POST, (double)npart + (2.0 * d + 2.0) * nreg * (2.0 * nreg + 4.0 * N),
		             8.0 * ((double)npart + (2.0 * d + 2.0) * 3.0 * N * nreg));
		HIPCHK(ctx, launch_sens_post_finish(ctx->stream, ctx->dSensPostPart, N, d, ctx->order, nreg, ctx->pred_cov.amp, ctx->dSensPrep,
		                                    ctx->dSensCst, ctx->dSensG, Q, out_dev));
	}
	ctx->sens_post_N = N;
	return GPEMU_OK;
}

extern "C" int gpemu_sens_post(gpemu_ctx *ctx, const double *lo, const double *hi, double *s_none, double *s_all, double *s_first,
                               double *s_rest)
{
	if (!ctx || !lo || !hi || !s_none || !s_all || !s_first || !s_rest) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_check(ctx, ctx, lo, hi, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t d = (size_t)ctx->d;
	if (const int rc = grow(ctx, ctx->dSensOut, 3 + 2 * (size_t)GPEMU_MAX_PARAMS)) return rc;
	if (const int rc = gpemu_sens_post_dev(ctx, lo, hi, ctx->dSensOut)) return rc;
	std::vector<double> o(2 + 2 * d);
	HIPCHK(ctx, hipMemcpyAsync(o.data(), ctx->dSensOut, o.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	*s_none = o[0];
	*s_all = o[1];
	memcpy(s_first, o.data() + 2, d * sizeof(double));
	memcpy(s_rest, o.data() + 2 + d, d * sizeof(double));
	return GPEMU_OK;
}

// The confidence band of the main-effect curves: the prediction's variance formula with T for the k-vector.  Blocks of up to
// PRED_BATCH_MAX of the d ngrid + 1 rows through dKq and dV in stream order, as gpemu_predict_cov_dev uses them; K is never
// split (few rows take the same 64-row tiles, so a row's bits do not depend on ngrid).
extern "C" int gpemu_sens_main_var(gpemu_ctx *ctx, const double *lo, const double *hi, int ngrid, const double *grid, double *main,
                                   double *var, double *var_e0)
{
	if (!ctx || !lo || !hi || !grid || !var || ngrid < 1) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_check(ctx, ctx, lo, hi, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int N = ctx->N, d = ctx->d, Np = ctx->Np, Rp = ctx->Rp;
	const size_t ng = (size_t)d * ngrid, M = ng + 1;
	const int cap = (int)std::min((size_t)PRED_BATCH_MAX, (M + 63) / 64 * 64);
	int rc = grow(ctx, ctx->dSensGrid, ng + 2 * M);
	if (!rc) rc = ensure_pred_batch(ctx, cap);
	if (rc) return rc;
	double *dgrid = ctx->dSensGrid, *dmain = dgrid + ng, *dvar = dmain + M;
	HIPCHK(ctx, hipMemcpyAsync(dgrid, grid, ng * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (prof_on(ctx, GPEMU_PROF_SENS_POST)) ctx->prof.tag.push_back("sens_prep");
	if ((rc = sens_prep(ctx, bx, GPEMU_PROF_SENS_POST))) return rc;
	const long ldv = (long)Np + Rp;
	for (size_t r0 = 0; r0 < M; r0 += cap) {
		const int mb = (int)std::min((size_t)cap, M - r0), mbp = round_up(mb, 64);
		if (prof_on(ctx, GPEMU_PROF_SENS_POST)) for (const char *t : {"sens_tvec", "sens_band_finish"}) ctx->prof.tag.push_back(t);
		{
			ProfScope ps(ctx, GPEMU_PROF_SENS_POST, 6.0 * mb * (double)N, 8.0 * (double)mbp * Np);
			HIPCHK(ctx, launch_sens_tvec(ctx->stream, ctx->dX, N, Np, d, ctx->pred_cov.amp, ctx->dSensPrep, ctx->dSensCst, dgrid, ngrid,
			                             (int)r0, mb, mbp, ctx->dKq));
		}
		HIPCHK(ctx, launch_aug_product(ctx, aug_product_args(ctx, mb)));
		{
			ProfScope ps(ctx, GPEMU_PROF_SENS_POST, (double)mb * (2.0 * Np + 2.0 * ctx->nreg * ctx->nreg), 8.0 * (double)mb * (double)ldv);
			HIPCHK(ctx, launch_sens_band_finish(ctx->stream, ctx->dV, ldv, mb, (int)r0, Np, ctx->nreg, d, ngrid, ctx->dSensCst, dgrid,
			                                    ctx->dBetaQ, ctx->pred_cov.amp, dmain, dvar));
		}
	}
	if (main) HIPCHK(ctx, hipMemcpyAsync(main, dmain, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(var, dvar, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (var_e0) HIPCHK(ctx, hipMemcpyAsync(var_e0, dvar + ng, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// P (N x N, both triangles), G = W Q (N x nreg) and Q (nreg x nreg) exactly as the last gpemu_sens_post left and read them
// (parity tests: the reference starts from the bits the weighted sweep and its finish multiply by)
extern "C" int gpemu_test_sens_post_state(gpemu_ctx *ctx, double *P, double *G, double *Q)
{
	if (!ctx || !P || !G || !Q) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->sens_post_N != ctx->N || !ctx->dSensP) return fail(ctx, GPEMU_ERR_STATE, "gpemu_sens_post has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t N = (size_t)ctx->N, nreg = (size_t)ctx->nreg, ldp = (size_t)round_up(ctx->N, 64);
	// row i' of the buffer holds P_ii' for every i of the tiles at and below its own: the upper triangle of the output
	HIPCHK(ctx, hipMemcpy2DAsync(P, N * sizeof(double), ctx->dSensP, ldp * sizeof(double), N * sizeof(double), N, hipMemcpyDeviceToHost,
	                             ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(G, ctx->dSensG, N * nreg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(Q, ctx->dBetaQ + nreg, nreg * nreg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	for (size_t i = 0; i < N; i++)
		for (size_t j = i + 1; j < N; j++) P[j * N + i] = P[i * N + j];
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// expected reduction of the IMSE by one more run at each of M candidates (gpemu.h).  The tables of the design
// and [K ; HK], Hm (kept while the set-up, the box and the kinds stay); then per block of up to PRED_BATCH_MAX candidates, through
// dKq and dV in stream order as gpemu_predict_cov_dev uses them: the candidates' own tables, the unclamped k rows, V = Kq LinvAug^T
// and Q r as in gpemu_predict_var_grad_dev (K never split), that entry's second product for a^T, its transpose, T = a [K | HK],
// the cross sweep and the finish.  Everything else it writes is its own (dDesign*) or the sensitivity entries' tables.
// ---------------------------------------------------------------------------
static int design_check(gpemu_ctx *ctx, const double *lo, const double *hi, int npoints, const void *xq, const void *gain, SensBox *bx)
{
	if (!ctx || !lo || !hi || !xq || !gain || npoints < 1) return GPEMU_ERR_ARG;
	return sens_check(ctx, ctx, lo, hi, bx);
}

extern "C" int gpemu_design_gain_dev(gpemu_ctx *ctx, const double *lo, const double *hi, int npoints, const double *xq_dev, double *gain_dev,
                                     double *num_dev, double *var_dev)
{
	SensBox bx;
	if (const int rc = design_check(ctx, lo, hi, npoints, xq_dev, gain_dev, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int N = ctx->N, d = ctx->d, Np = ctx->Np, Rp = ctx->Rp, nreg = ctx->nreg, M = npoints;
	const int cap = std::min(PRED_BATCH_MAX, round_up(M, 64)), ntc = (N + 63) / 64;
	const long ldv = (long)Np + Rp, ldt = (long)Np + 64;
	if (ctx->dDesignKH.size() < design_kh_elems(Np) || ctx->dDesignHm.size() < 64 * 64) ctx->design_serial = 0;
	int rc = ensure_pred_batch(ctx, cap);
	if (!rc) rc = grow(ctx, ctx->dDesignKH, design_kh_elems(Np), false, "out of device memory for the design's pair integrals (8 Np (Np + 64) bytes)");
	if (!rc) rc = grow(ctx, ctx->dDesignHm, 64 * 64);
	if (!rc) rc = grow(ctx, ctx->dDesignPrepQ, sens_prep_elems(cap, d));
	if (!rc) rc = grow(ctx, ctx->dDesignA, (size_t)cap * Np);
	if (!rc) rc = grow(ctx, ctx->dDesignT, (size_t)cap * ldt);
	if (!rc) rc = grow(ctx, ctx->dDesignR, (size_t)cap * Rp);
	if (!rc) rc = grow(ctx, ctx->dDesignB, (size_t)cap * 64);
	if (!rc) rc = grow(ctx, ctx->dDesignPart, (size_t)ntc * cap);
	if (!rc) rc = ensure_linv_transposed(ctx);
	if (rc) return rc;
	const bool prof = prof_on(ctx, GPEMU_PROF_DESIGN);
	if (prof) ctx->prof.tag.push_back("sens_prep");
	if ((rc = sens_prep(ctx, bx, GPEMU_PROF_DESIGN))) return rc;
	if (ctx->design_serial != ctx->pred_serial || memcmp(&ctx->design_box, &bx, sizeof bx) != 0) {
		ctx->design_serial = 0;
		if (prof) ctx->prof.tag.push_back("design_kmat");
		// per pair of the lower tiles d pair factors; K, its mirror image and the HK rows written
		ProfScope ps(ctx, GPEMU_PROF_DESIGN, 0.5 * N * (double)N * sens_pair_flops(bx, d), 8.0 * (double)design_kh_elems(Np));
		HIPCHK(ctx, launch_design_kmat(ctx->stream, ctx->dX, N, Np, d, nreg, ctx->dSensPrep, ctx->dSensCst, bx.meas, ctx->dDesignKH,
		                               ctx->dDesignHm));
		ctx->design_serial = ctx->pred_serial;
		ctx->design_box = bx;
	}
	for (int q0 = 0; q0 < M; q0 += cap) {
		const int mb = std::min(cap, M - q0), mbp = round_up(mb, 64);
		const double *xq = xq_dev + (size_t)q0 * d;
		if (prof) for (const char *t : {"sens_prep_candidates", "design_kvec"}) ctx->prof.tag.push_back(t);
		{
			ProfScope ps(ctx, GPEMU_PROF_DESIGN, 2.0 * mb * d * 44.0, 8.0 * ((double)sens_prep_elems(mb, d) + (double)mb * d));
			HIPCHK(ctx, launch_sens_prep(ctx->stream, xq, mb, bx, ctx->dDesignPrepQ, ctx->dSensCst));
		}
		{
			ProfScope ps(ctx, GPEMU_PROF_DESIGN, (double)mb * N * (3.0 * d + 2.0), 8.0 * (double)mbp * Np);
			HIPCHK(ctx, launch_design_kvec(ctx->stream, ctx->dX, N, Np, d, ctx->dSensCst, ctx->pred_cov.amp, xq, mb, mbp, ctx->dKq));
		}
		HIPCHK(ctx, launch_aug_product(ctx, aug_product_args(ctx, mb)));
		HIPCHK(ctx, launch_predict_qr(ctx->stream, ctx->dV, ldv, mb, Np, Rp, nreg, d, xq, ctx->dBetaQ, ctx->dDesignR));
		// a^T (Np x mbp) = LinvAugT . [u | 0 | Q r]^T, exactly the second product of gpemu_predict_var_grad_dev
		GemmArgs t{};
		t.C = ctx->dKq; t.ldc = mbp;
		t.A = ctx->dLinvAugT; t.lda = ldv;
		t.B = ctx->dV; t.ldb = ldv;
		t.m = Np; t.n = mb; t.k0 = 0; t.k1 = Np + Rp; t.alpha = 1.0; t.beta = 0;
		t.kstart_mode = 1; t.kstart_off = 0;
		HIPCHK(ctx, gemm(ctx, t));
		if (prof) ctx->prof.tag.push_back("design_transpose");
		{
			ProfScope ps(ctx, GPEMU_PROF_DESIGN, 0.0, 16.0 * (double)mbp * Np);
			HIPCHK(ctx, launch_transpose_rect(ctx->stream, ctx->dDesignA, Np, ctx->dKq, mbp, Np, mbp));
		}
		// T (mb x (Np + 64)) = a [K | HK]
		GemmArgs g{};
		g.C = ctx->dDesignT; g.ldc = ldt;
		g.A = ctx->dDesignA; g.lda = Np;
		g.B = ctx->dDesignKH; g.ldb = Np;
		g.m = mb; g.n = Np + 64; g.k0 = 0; g.k1 = Np; g.alpha = 1.0; g.beta = 0;
		HIPCHK(ctx, gemm(ctx, g));
		if (prof) for (const char *t2 : {"design_cross", "design_finish"}) ctx->prof.tag.push_back(t2);
		{
			// per pair d pair factors and the fused multiply-add; a and T read, one partial per candidate and tile column written
			ProfScope ps(ctx, GPEMU_PROF_DESIGN, (double)mb * N * (sens_pair_flops(bx, d) + 4.0), 8.0 * (double)mb * (2.0 * N + ntc));
			HIPCHK(ctx, launch_design_cross(ctx->stream, ctx->dX, N, d, xq, mb, ctx->dSensCst, bx.meas, ctx->dDesignA, Np, ctx->dDesignT, ldt,
			                                ctx->dDesignPart, cap));
		}
		{
			ProfScope ps(ctx, GPEMU_PROF_DESIGN, (double)mb * (2.0 * Np + 2.0 * nreg * nreg + sens_pair_flops(bx, d)), 8.0 * (double)mb * (double)ldv);
			HIPCHK(ctx, launch_design_finish(ctx->stream, ctx->dDesignPart, cap, N, ctx->dV, ldv, ctx->dDesignR, Rp, ctx->dDesignT, ldt,
			                                 ctx->dDesignPrepQ, xq, mb, Np, d, nreg, ctx->dSensCst, bx.meas, ctx->dDesignHm, ctx->pred_cov.amp,
			                                 ctx->kappa, gain_dev + q0, num_dev ? num_dev + q0 : nullptr, var_dev ? var_dev + q0 : nullptr,
			                                 ctx->dDesignB));
		}
		ctx->design_mb = mb;
	}
	return GPEMU_OK;
}

// host buffers: candidates and results through a buffer of the entry's own, so that a pending prediction batch keeps its staging
extern "C" int gpemu_design_gain(gpemu_ctx *ctx, const double *lo, const double *hi, int npoints, const double *xq, double *gain, double *num,
                                 double *var)
{
	SensBox bx;
	if (const int rc = design_check(ctx, lo, hi, npoints, xq, gain, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t M = (size_t)npoints, d = (size_t)ctx->d;
	if (const int rc = grow(ctx, ctx->dDesignOut, M * (d + 3))) return rc;
	double *dx = ctx->dDesignOut, *dg = dx + M * d, *dn = dg + M, *dv = dn + M;
	HIPCHK(ctx, hipMemcpyAsync(dx, xq, M * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (const int rc = gpemu_design_gain_dev(ctx, lo, hi, npoints, dx, dg, dn, dv)) return rc;
	HIPCHK(ctx, hipMemcpyAsync(gain, dg, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (num) HIPCHK(ctx, hipMemcpyAsync(num, dn, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (var) HIPCHK(ctx, hipMemcpyAsync(var, dv, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// a (npoints x N) and b (npoints x nreg) exactly as the last block of the last gpemu_design_gain read them (parity tests: the
// reference starts from the bits the products and the sweep multiplied by); npoints: that block's candidates
extern "C" int gpemu_test_design_state(gpemu_ctx *ctx, int npoints, double *a_out, double *b_out)
{
	if (!ctx || !a_out || !b_out || npoints < 1) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->design_mb != npoints || !ctx->dDesignA || !ctx->dDesignB || ctx->design_serial != ctx->pred_serial)
		return fail(ctx, GPEMU_ERR_STATE, "no gpemu_design_gain block of this size");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t N = (size_t)ctx->N, nreg = (size_t)ctx->nreg, Np = (size_t)ctx->Np;
	HIPCHK(ctx, hipMemcpy2DAsync(a_out, N * sizeof(double), ctx->dDesignA, Np * sizeof(double), N * sizeof(double), (size_t)npoints,
	                             hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(b_out, nreg * sizeof(double), ctx->dDesignB, 64 * sizeof(double), nreg * sizeof(double), (size_t)npoints,
	                             hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// greedy batches of nbatch runs (gpemu.h).  Per context, on its own stream: the first pass is one block of
// gpemu_design_gain_dev, with num, var and gain landing in the running state (dBatchSt), then the rows of w; per pick the
// gather, the column kernel and the update.  The arg-max over the weighted gains runs on ctxs[0]'s stream, which waits on the
// other streams by events (each context's sens_ev); they wait on its event (ctxs[0]'s sens_ev2) before they read the pick.
// The host takes no part between picks.
// ---------------------------------------------------------------------------
static int design_batch_check(gpemu_ctx *const *ctxs, int nctx, const double *weight, const double *lo, const double *hi, int npoints,
                              const void *xq, int nbatch, const void *pick, const void *pick_gain, std::vector<SensBox> *bxs)
{
	if (!ctxs || nctx < 1 || !lo || !hi || !xq || !pick || !pick_gain) return GPEMU_ERR_ARG;
	for (int c = 0; c < nctx; c++)
		if (!ctxs[c]) return GPEMU_ERR_ARG;
	if (npoints < 1 || npoints > PRED_BATCH_MAX || nbatch < 1 || nbatch > std::min(npoints, 256)) return GPEMU_ERR_ARG;
	gpemu_ctx *lead = ctxs[0];
	for (int c = 0; c < nctx; c++)
		if (!ctxs[c]->pred_ready) return fail(lead, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	bxs->resize(nctx);
	for (int c = 0; c < nctx; c++) {
		SensBox pair;
		if (const int rc = sens_check(lead, ctxs[c], lo, hi, &pair)) return rc;       // the same design, order, kinds and device
		if (const int rc = sens_check(ctxs[c], ctxs[c], lo, hi, &(*bxs)[c])) return rc;
		for (int e = 0; e < c; e++)
			if (ctxs[e] == ctxs[c]) return fail(lead, GPEMU_ERR_ARG, "design batch: a context is listed twice");
	}
	for (int c = 0; weight && c < nctx; c++)
		if (!std::isfinite(weight[c]) || weight[c] < 0.0) return fail(lead, GPEMU_ERR_ARG, "design batch: a weight must be finite and >= 0");
	return GPEMU_OK;
}

extern "C" int gpemu_design_batch_dev(gpemu_ctx *const *ctxs, int nctx, const double *weight, const double *lo, const double *hi, int npoints,
                                      const double *xq_dev, int nbatch, int *pick_dev, double *pick_gain_dev, double *pick_gain_ctx_dev,
                                      double *gain_first_dev, double *gain_last_dev)
{
	std::vector<SensBox> bxs;
	if (const int rc = design_batch_check(ctxs, nctx, weight, lo, hi, npoints, xq_dev, nbatch, pick_dev, pick_gain_dev, &bxs)) return rc;
	gpemu_ctx *lead = ctxs[0];
	HIPCHK(lead, hipSetDevice(lead->device));
	const int M = npoints, mbp = round_up(M, 64), N = lead->N, d = lead->d, Np = lead->Np, nreg = lead->nreg;
	const long ldt = (long)Np + 64, ldl = nbatch;
	HIPCHK(lead, hipStreamSynchronize(lead->stream));                                 // (an earlier call's arg-max may still read the contexts' gains)
	for (int c = 0; c < nctx; c++) {
		gpemu_ctx *ctx = ctxs[c];
		ctx->batch_mb = ctx->batch_nb = 0;
		int rc = grow(ctx, ctx->dBatchW, (size_t)mbp * Np, false, "out of device memory for the rows of w (8 M' Np bytes)");
		if (!rc) rc = grow(ctx, ctx->dBatchLam, (size_t)M * nbatch);
		if (!rc) rc = grow(ctx, ctx->dBatchMu, (size_t)M * nbatch);
		if (!rc) rc = grow(ctx, ctx->dBatchE, 256 * 256);
		if (!rc) rc = grow(ctx, ctx->dBatchSv, design_batch_sv_elems(Np));
		if (!rc) rc = grow(ctx, ctx->dBatchDots, 4 * (size_t)M);
		if (!rc) rc = grow(ctx, ctx->dBatchSt, 3 * (size_t)M);
		if (!rc && !ctx->sens_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sens_ev, hipEventDisableTiming));
		if (!rc && !ctx->sens_ev2) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sens_ev2, hipEventDisableTiming));
		if (rc) return rc;
	}
	// the table of the arg-max: the contexts' gain pointers, the weights, the picked marks (ints)
	const size_t tab = 2 * (size_t)nctx + ((size_t)M + 1) / 2;
	if (const int rc = grow(lead, lead->dBatchTab, tab)) return rc;
	HIPCHK(lead, hipStreamSynchronize(lead->stream));                                 // (an earlier call's launches may still read the table)
	{
		std::vector<double> h(2 * (size_t)nctx);
		for (int c = 0; c < nctx; c++) {
			const double *g = ctxs[c]->dBatchSt + 2 * (size_t)M;
			memcpy(&h[c], &g, sizeof g);
			h[nctx + c] = weight ? weight[c] : 1.0;
		}
		HIPCHK(lead, hipMemcpy(lead->dBatchTab, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
	}
	const double *const *gains = reinterpret_cast<const double *const *>((double *)lead->dBatchTab);
	const double *wdev = lead->dBatchTab + nctx;
	int *picked = reinterpret_cast<int *>(lead->dBatchTab + 2 * (size_t)nctx);
	HIPCHK(lead, hipMemsetAsync(picked, 0, (size_t)M * sizeof(int), lead->stream));
	// the other streams behind what ctxs[0]'s stream holds (the caller's candidates among it)
	HIPCHK(lead, hipEventRecord(lead->sens_ev2, lead->stream));
	for (int c = 1; c < nctx; c++) HIPCHK(lead, hipStreamWaitEvent(ctxs[c]->stream, lead->sens_ev2, 0));
	for (int c = 0; c < nctx; c++) {
		gpemu_ctx *ctx = ctxs[c];
		double *st = ctx->dBatchSt;
		if (const int rc = gpemu_design_gain_dev(ctx, lo, hi, M, xq_dev, st + 2 * (size_t)M, st + M, st)) return rc;
		const bool prof = prof_on(ctx, GPEMU_PROF_DESIGN);
		if (prof) ctx->prof.tag.push_back("design_wrows");
		ProfScope ps(ctx, GPEMU_PROF_DESIGN, (double)M * N * sens_pair_flops(bxs[c], d), 8.0 * (double)mbp * Np);
		HIPCHK(ctx, launch_design_wrows(ctx->stream, ctx->dX, N, Np, d, ctx->dSensCst, bxs[c].meas, xq_dev, M, mbp, ctx->dBatchW));
	}
	for (int j = 0; j <= nbatch; j++) {
		// the arg-max of pick j (j = nbatch: only gain_last) behind every context's update
		for (int c = 1; c < nctx; c++) {
			HIPCHK(lead, hipEventRecord(ctxs[c]->sens_ev, ctxs[c]->stream));
			HIPCHK(lead, hipStreamWaitEvent(lead->stream, ctxs[c]->sens_ev, 0));
		}
		double *wout = j == 0 ? gain_first_dev : (j == nbatch ? gain_last_dev : nullptr);
		if (j < nbatch || wout) {
			if (prof_on(lead, GPEMU_PROF_DESIGN)) lead->prof.tag.push_back("design_argmax");
			ProfScope ps(lead, GPEMU_PROF_DESIGN, 2.0 * nctx * M, 8.0 * (nctx + 1.0) * M);
			HIPCHK(lead, launch_design_argmax(lead->stream, gains, wdev, nctx, M, picked, j < nbatch ? j : -1, pick_dev, pick_gain_dev,
			                                  pick_gain_ctx_dev, wout));
		}
		if (j == nbatch) break;
		HIPCHK(lead, hipEventRecord(lead->sens_ev2, lead->stream));
		for (int c = 0; c < nctx; c++) {
			gpemu_ctx *ctx = ctxs[c];
			if (c) HIPCHK(lead, hipStreamWaitEvent(ctx->stream, lead->sens_ev2, 0));
			double *st = ctx->dBatchSt;
			const bool prof = prof_on(ctx, GPEMU_PROF_DESIGN);
			if (prof) ctx->prof.tag.push_back("design_gather");
			{
				ProfScope ps(ctx, GPEMU_PROF_DESIGN, (double)N * (3.0 * d + 2.0), 8.0 * 5.0 * Np);
				HIPCHK(ctx, launch_design_gather(ctx->stream, pick_dev, j, ctx->dX, N, Np, d, nreg, ctx->dSensCst, ctx->pred_cov.amp, xq_dev, M,
				                                 ctx->dDesignA, ctx->dDesignT, ldt, ctx->dBatchW, ctx->dDesignB, ctx->dDesignPrepQ, ctx->dDesignHm,
				                                 ctx->dBatchLam, ctx->dBatchMu, ldl, st, st + M, ctx->dBatchE, ctx->dBatchSv));
			}
			if (prof) ctx->prof.tag.push_back("design_column");
			{
				// four fused multiply-adds per column; the rows of a, T^K and w read once
				ProfScope ps(ctx, GPEMU_PROF_DESIGN, 8.0 * (double)M * Np, 8.0 * 3.0 * (double)M * Np);
				HIPCHK(ctx, launch_design_column(ctx->stream, ctx->dDesignA, ctx->dDesignT, ldt, ctx->dBatchW, Np, M, ctx->dBatchSv,
				                                 ctx->dBatchDots, M));
			}
			if (prof) ctx->prof.tag.push_back("design_update");
			{
				ProfScope ps(ctx, GPEMU_PROF_DESIGN, (double)M * (12.0 * nreg + 6.0 * j + sens_pair_flops(bxs[c], d)),
				             8.0 * (double)M * (2.0 * nreg + 2.0 * j + 12.0));
				HIPCHK(ctx, launch_design_update(ctx->stream, j, xq_dev, M, Np, d, nreg, ctx->dSensCst, bxs[c].meas, ctx->pred_cov.amp,
				                                 ctx->dDesignT, ldt, ctx->dDesignB, ctx->dDesignPrepQ, ctx->dBatchSv, ctx->dBatchDots, M,
				                                 ctx->dBatchLam, ctx->dBatchMu, ldl, st, st + M, st + 2 * (size_t)M));
			}
		}
	}
	for (int c = 0; c < nctx; c++) {
		ctxs[c]->batch_mb = M;
		ctxs[c]->batch_nb = nbatch;
	}
	return GPEMU_OK;
}

// host buffers: the candidates and the results through a buffer of ctxs[0]'s own
extern "C" int gpemu_design_batch(gpemu_ctx *const *ctxs, int nctx, const double *weight, const double *lo, const double *hi, int npoints,
                                  const double *xq, int nbatch, int *pick, double *pick_gain, double *pick_gain_ctx, double *gain_first,
                                  double *gain_last)
{
	std::vector<SensBox> bxs;
	if (const int rc = design_batch_check(ctxs, nctx, weight, lo, hi, npoints, xq, nbatch, pick, pick_gain, &bxs)) return rc;
	gpemu_ctx *lead = ctxs[0];
	HIPCHK(lead, hipSetDevice(lead->device));
	const size_t M = (size_t)npoints, d = (size_t)lead->d, nb = (size_t)nbatch, nc = (size_t)nctx;
	if (const int rc = grow(lead, lead->dBatchIO, M * (d + 2) + nb * (nc + 1) + (nb + 1) / 2)) return rc;
	double *dx = lead->dBatchIO, *dgf = dx + M * d, *dgl = dgf + M, *dpg = dgl + M, *dpc = dpg + nb;
	int *dpk = reinterpret_cast<int *>(dpc + nb * nc);
	HIPCHK(lead, hipMemcpyAsync(dx, xq, M * d * sizeof(double), hipMemcpyHostToDevice, lead->stream));
	if (const int rc = gpemu_design_batch_dev(ctxs, nctx, weight, lo, hi, npoints, dx, nbatch, dpk, dpg, pick_gain_ctx ? dpc : nullptr,
	                                          gain_first ? dgf : nullptr, gain_last ? dgl : nullptr))
		return rc;
	HIPCHK(lead, hipMemcpyAsync(pick, dpk, nb * sizeof(int), hipMemcpyDeviceToHost, lead->stream));
	HIPCHK(lead, hipMemcpyAsync(pick_gain, dpg, nb * sizeof(double), hipMemcpyDeviceToHost, lead->stream));
	if (pick_gain_ctx) HIPCHK(lead, hipMemcpyAsync(pick_gain_ctx, dpc, nb * nc * sizeof(double), hipMemcpyDeviceToHost, lead->stream));
	if (gain_first) HIPCHK(lead, hipMemcpyAsync(gain_first, dgf, M * sizeof(double), hipMemcpyDeviceToHost, lead->stream));
	if (gain_last) HIPCHK(lead, hipMemcpyAsync(gain_last, dgl, M * sizeof(double), hipMemcpyDeviceToHost, lead->stream));
	HIPCHK(lead, hipStreamSynchronize(lead->stream));
	return GPEMU_OK;
}

// lambda and mu (npoints x nbatch each) and E (nbatch x nbatch) of the context's part in the last gpemu_design_batch, bit for bit
extern "C" int gpemu_test_design_batch_state(gpemu_ctx *ctx, int npoints, int nbatch, double *lam_out, double *mu_out, double *e_out)
{
	if (!ctx || !lam_out || !mu_out || !e_out || npoints < 1 || nbatch < 1) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->batch_mb != npoints || ctx->batch_nb != nbatch || !ctx->dBatchLam || !ctx->dBatchE || ctx->design_serial != ctx->pred_serial)
		return fail(ctx, GPEMU_ERR_STATE, "no gpemu_design_batch of this size");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t n = (size_t)npoints * nbatch * sizeof(double), row = (size_t)nbatch * sizeof(double);
	HIPCHK(ctx, hipMemcpyAsync(lam_out, ctx->dBatchLam, n, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(mu_out, ctx->dBatchMu, n, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(e_out, row, ctx->dBatchE, 256 * sizeof(double), row, (size_t)nbatch, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// gain over a weighted set of target points (gpemu.h).  The store of the targets -- u, r and Q r per target, v(x_s)
// and the target variance -- is built per block of up to PRED_BATCH_MAX targets through dKq and dV in stream order, by the chain of
// gpemu_design_gain_dev from its k fill to launch_predict_qr with the fill of every covariance function in its place (mode 0, nugget
// 0), and copied out of dV; it belongs to one prediction set-up (tgt_serial) and is rebuilt from the kept coordinates by the first
// gain call after another.  Per block of candidates the same chain, then per panel of target columns P = U_q U_t^T on the GEMM,
// the sweep and the finish.  Everything else written is the entries' own (dTgt*).
// ---------------------------------------------------------------------------
constexpr int TARGET_MAX = 65536;

// the covariance parameters of the set-up without the nugget: c(., .) is the bare kernel value wherever two points lie
static CovParams target_cov(const gpemu_ctx *ctx)
{
	CovParams p = ctx->pred_cov;
	p.nug = 0.0;
	return p;
}

// the chain both halves share, for the mb points xq (device): unclamped k rows, V = Kq LinvAug^T, the variance with c(x, x) =
// kappa, then Q r into V's columns Np .. with r kept in rkeep
static int target_chain(gpemu_ctx *ctx, const CovParams &p, const double *xq, int mb, double kappa, double *mean_scratch, double *var_out,
                        double *rkeep)
{
	const int N = ctx->N, d = ctx->d, Np = ctx->Np, Rp = ctx->Rp, mbp = round_up(mb, 64);
	const long ldv = (long)Np + Rp;
	if (prof_on(ctx, GPEMU_PROF_DESIGN_TARGET)) ctx->prof.tag.push_back("target_kvec");
	{
		ProfScope ps(ctx, GPEMU_PROF_DESIGN_TARGET, (double)mb * N * (3.0 * d + 2.0), 8.0 * (double)mbp * Np);
		HIPCHK(ctx, launch_cov_fill(ctx->stream, ctx->dKq, Np, xq, mb, mbp, ctx->dX, N, Np, d, p, 0));
	}
	HIPCHK(ctx, launch_aug_product(ctx, aug_product_args(ctx, mb)));
	HIPCHK(ctx, launch_predict_finish(ctx->stream, ctx->dV, ldv, mb, Np, ctx->nreg, ctx->order, d, xq, ctx->dBetaQ, kappa, mean_scratch, var_out, 1,
	                                  (long)mbp * ldv));
	HIPCHK(ctx, launch_predict_qr(ctx->stream, ctx->dV, ldv, mb, Np, Rp, ctx->nreg, d, xq, ctx->dBetaQ, rkeep));
	return GPEMU_OK;
}

// the store of the tgt_S targets in dTgtX / dTgtW for the present set-up
static int target_build(gpemu_ctx *ctx)
{
	const int S = ctx->tgt_S, d = ctx->d, Np = ctx->Np, Rp = ctx->Rp, Sp = round_up(S, 64);
	const int cap = std::min(PRED_BATCH_MAX, Sp);
	const long ldv = (long)Np + Rp;
	ctx->tgt_serial = 0;
	int rc = ensure_pred_batch(ctx, cap);
	if (!rc) rc = grow(ctx, ctx->dTgtU, (size_t)Sp * Np, false, "out of device memory for the targets' u rows (8 S' Np bytes)");
	if (!rc) rc = grow(ctx, ctx->dTgtR, (size_t)Sp * Rp);
	if (!rc) rc = grow(ctx, ctx->dTgtQr, (size_t)Sp * Rp);
	if (!rc) rc = grow(ctx, ctx->dTgtVar, (size_t)Sp);
	if (!rc) rc = grow(ctx, ctx->dTgtSum, 1);
	if (!rc) rc = grow(ctx, ctx->dTgtScr, 3 * (size_t)cap);
	if (rc) return rc;
	const CovParams p = target_cov(ctx);
	for (int s0 = 0; s0 < S; s0 += cap) {
		const int mb = std::min(cap, S - s0);
		// v(x_s) is latent: c(x_s, x_s) = the amplitude, no nugget
		if ((rc = target_chain(ctx, p, ctx->dTgtX + (size_t)s0 * d, mb, p.amp, ctx->dTgtScr, ctx->dTgtVar + s0, ctx->dTgtR + (size_t)s0 * Rp)))
			return rc;
		HIPCHK(ctx, hipMemcpy2DAsync(ctx->dTgtU + (size_t)s0 * Np, (size_t)Np * sizeof(double), ctx->dV, (size_t)ldv * sizeof(double),
		                             (size_t)Np * sizeof(double), (size_t)mb, hipMemcpyDeviceToDevice, ctx->stream));
		HIPCHK(ctx, hipMemcpy2DAsync(ctx->dTgtQr + (size_t)s0 * Rp, (size_t)Rp * sizeof(double), ctx->dV + Np, (size_t)ldv * sizeof(double),
		                             (size_t)Rp * sizeof(double), (size_t)mb, hipMemcpyDeviceToDevice, ctx->stream));
	}
	if (prof_on(ctx, GPEMU_PROF_DESIGN_TARGET)) ctx->prof.tag.push_back("target_var");
	{
		ProfScope ps(ctx, GPEMU_PROF_DESIGN_TARGET, 2.0 * S, 16.0 * S);
		HIPCHK(ctx, launch_design_target_var(ctx->stream, ctx->dTgtW, ctx->dTgtVar, S, ctx->dTgtSum));
	}
	ctx->tgt_serial = ctx->pred_serial;
	ctx->tgt_mb = 0;
	return GPEMU_OK;
}

// weight: ntargets finite values >= 0 with a positive sum, or NULL
static bool target_weights_ok(int ntargets, const double *weight)
{
	if (!weight) return true;
	double sum = 0.0;
	for (int s = 0; s < ntargets; s++) {
		if (!std::isfinite(weight[s]) || weight[s] < 0.0) return false;
		sum += weight[s];
	}
	return sum > 0.0;
}

// both set entries behind their checks: xt in host or device memory, the results into host or device memory
static int target_set(gpemu_ctx *ctx, int S, const double *xt, bool host, const double *weight, double *target_var, double *var_t)
{
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int d = ctx->d, Sp = round_up(S, 64);
	ctx->tgt_S = 0;
	ctx->tgt_serial = 0;
	int rc = grow(ctx, ctx->dTgtX, (size_t)Sp * d);
	if (!rc) rc = grow(ctx, ctx->dTgtW, (size_t)Sp);
	if (rc) return rc;
	std::vector<double> w((size_t)S, 1.0 / S);
	if (weight) w.assign(weight, weight + S);
	HIPCHK(ctx, hipMemcpyAsync(ctx->dTgtX, xt, (size_t)S * d * sizeof(double), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dTgtW, w.data(), (size_t)S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));           // w is this call's own: its upload is waited for
	ctx->tgt_S = S;
	if ((rc = target_build(ctx))) return rc;
	const hipMemcpyKind out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	if (target_var) HIPCHK(ctx, hipMemcpyAsync(target_var, ctx->dTgtSum, sizeof(double), out, ctx->stream));
	if (var_t) HIPCHK(ctx, hipMemcpyAsync(var_t, ctx->dTgtVar, (size_t)S * sizeof(double), out, ctx->stream));
	if (host) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

extern "C" int gpemu_design_target_set_dev(gpemu_ctx *ctx, int ntargets, const double *xt_dev, const double *weight, double *target_var_dev,
                                           double *var_t_dev)
{
	if (!ctx || !xt_dev || ntargets < 1 || ntargets > TARGET_MAX || !target_weights_ok(ntargets, weight)) return GPEMU_ERR_ARG;
	return target_set(ctx, ntargets, xt_dev, false, weight, target_var_dev, var_t_dev);
}

extern "C" int gpemu_design_target_set(gpemu_ctx *ctx, int ntargets, const double *xt, const double *weight, double *target_var, double *var_t)
{
	if (!ctx || !xt || ntargets < 1 || ntargets > TARGET_MAX || !target_weights_ok(ntargets, weight)) return GPEMU_ERR_ARG;
	if (ctx->d > 0)
		for (size_t e = 0; e < (size_t)ntargets * ctx->d; e++)
			if (!std::isfinite(xt[e])) return fail(ctx, GPEMU_ERR_ARG, "design target: a coordinate is not finite");
	return target_set(ctx, ntargets, xt, true, weight, target_var, var_t);
}

extern "C" int gpemu_design_target_release(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	free_targets(ctx);
	return GPEMU_OK;
}

static int target_gain_check(gpemu_ctx *ctx, int npoints, const void *xq, const void *gain)
{
	if (!ctx || !xq || !gain || npoints < 1) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->tgt_S < 1) return fail(ctx, GPEMU_ERR_STATE, "gpemu_design_target_set has not been called");
	return GPEMU_OK;
}

extern "C" int gpemu_design_target_gain_dev(gpemu_ctx *ctx, int npoints, const double *xq_dev, double *gain_dev, double *num_dev, double *var_dev)
{
	if (const int rc = target_gain_check(ctx, npoints, xq_dev, gain_dev)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int d = ctx->d, Np = ctx->Np, Rp = ctx->Rp, nreg = ctx->nreg, M = npoints, S = ctx->tgt_S;
	const int cap = std::min(PRED_BATCH_MAX, round_up(M, 64)), pw = std::min(ctx->sched.target_panel, round_up(S, 64));
	const long ldv = (long)Np + Rp;
	int rc = ensure_pred_batch(ctx, cap);
	if (!rc) rc = grow(ctx, ctx->dTgtCR, (size_t)cap * Rp);
	if (!rc) rc = grow(ctx, ctx->dTgtPanel, (size_t)cap * pw, false, "out of device memory for a panel of the targets' product (8 M' panel bytes)");
	if (!rc) rc = grow(ctx, ctx->dTgtPart, (size_t)(pw / 64) * cap);
	if (!rc) rc = grow(ctx, ctx->dTgtScr, 3 * (size_t)cap);
	if (!rc && ctx->tgt_serial != ctx->pred_serial) rc = target_build(ctx);     // another set-up since: the store from the kept coordinates
	if (rc) return rc;
	const CovParams p = target_cov(ctx);
	const bool prof = prof_on(ctx, GPEMU_PROF_DESIGN_TARGET);
	double *scr_mean = ctx->dTgtScr, *scr_var = scr_mean + cap, *scr_num = scr_var + cap;
	for (int q0 = 0; q0 < M; q0 += cap) {
		const int mb = std::min(cap, M - q0);
		const double *xq = xq_dev + (size_t)q0 * d;
		double *var = var_dev ? var_dev + q0 : scr_var, *num = num_dev ? num_dev + q0 : scr_num;
		// var is the variance a run at x* is observed with: c(x*, x*) = kappa carries the nugget once
		if ((rc = target_chain(ctx, p, xq, mb, ctx->kappa, scr_mean, var, ctx->dTgtCR))) return rc;
		for (int s0 = 0; s0 < S; s0 += pw) {
			const int ns = std::min(pw, S - s0), ntile = (ns + 63) / 64;
			GemmArgs g{};
			g.C = ctx->dTgtPanel; g.ldc = pw;
			g.A = ctx->dV; g.lda = ldv;
			g.B = ctx->dTgtU + (size_t)s0 * Np; g.ldb = Np;
			g.m = mb; g.n = ns; g.k0 = 0; g.k1 = Np; g.alpha = 1.0; g.beta = 0;
			HIPCHK(ctx, gemm(ctx, g));
			if (prof) for (const char *t : {"target_sweep", "target_finish"}) ctx->prof.tag.push_back(t);
			{
				// per pair the squared distance (3 d), the kernel (about 20), the regression sum (2 nreg) and the square, weight and
				// sum (5); the panel read, one partial per candidate and tile written
				ProfScope ps(ctx, GPEMU_PROF_DESIGN_TARGET, (double)mb * ns * (3.0 * d + 2.0 * nreg + 25.0), 8.0 * (double)mb * (ns + ntile));
				HIPCHK(ctx, launch_design_target_sweep(ctx->stream, xq, mb, ctx->dTgtX, S, s0, ns, d, p, ctx->dTgtPanel, pw, ctx->dTgtCR, Rp,
				                                       ctx->dTgtQr, Rp, ctx->dTgtW, nreg, ctx->dTgtPart, cap));
			}
			{
				ProfScope ps(ctx, GPEMU_PROF_DESIGN_TARGET, (double)mb * ntile, 8.0 * (double)mb * (ntile + 3));
				HIPCHK(ctx, launch_design_target_finish(ctx->stream, ctx->dTgtPart, cap, ntile, mb, s0 == 0, s0 + pw >= S, var, num, gain_dev + q0));
			}
		}
		ctx->tgt_mb = mb;
	}
	return GPEMU_OK;
}

// host buffers: candidates and results through a buffer of the entry's own, so that a pending prediction batch keeps its staging
extern "C" int gpemu_design_target_gain(gpemu_ctx *ctx, int npoints, const double *xq, double *gain, double *num, double *var)
{
	if (const int rc = target_gain_check(ctx, npoints, xq, gain)) return rc;
	const size_t M = (size_t)npoints, d = (size_t)ctx->d;
	for (size_t e = 0; e < M * d; e++)
		if (!std::isfinite(xq[e])) return fail(ctx, GPEMU_ERR_ARG, "design target: a coordinate is not finite");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (const int rc = grow(ctx, ctx->dTgtIO, M * (d + 3))) return rc;
	double *dx = ctx->dTgtIO, *dg = dx + M * d, *dn = dg + M, *dv = dn + M;
	HIPCHK(ctx, hipMemcpyAsync(dx, xq, M * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (const int rc = gpemu_design_target_gain_dev(ctx, npoints, dx, dg, dn, dv)) return rc;
	HIPCHK(ctx, hipMemcpyAsync(gain, dg, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (num) HIPCHK(ctx, hipMemcpyAsync(num, dn, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (var) HIPCHK(ctx, hipMemcpyAsync(var, dv, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// u (npoints x N), r and Q r (npoints x nreg each) bit for bit as the sweep reads them (parity tests): which = 0 the resident
// store of the npoints targets, which = 1 the last block of candidates of the last gain call -- its u and Q r rows are read out of
// the prediction batch buffer, so the call has to follow that gain call directly
extern "C" int gpemu_test_design_target_state(gpemu_ctx *ctx, int which, int npoints, double *u_out, double *r_out, double *qr_out)
{
	if (!ctx || !u_out || !r_out || !qr_out || npoints < 1 || which < 0 || which > 1) return GPEMU_ERR_ARG;
	if (!ctx->pred_ready) return fail(ctx, GPEMU_ERR_STATE, "gpemu_predict_setup has not been called");
	if (ctx->tgt_serial != ctx->pred_serial || (which == 0 ? ctx->tgt_S : ctx->tgt_mb) != npoints)
		return fail(ctx, GPEMU_ERR_STATE, which == 0 ? "no target set of this size" : "no gpemu_design_target_gain block of this size");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t N = (size_t)ctx->N, nreg = (size_t)ctx->nreg, Np = (size_t)ctx->Np, Rp = (size_t)ctx->Rp, ldv = Np + Rp;
	const double *u = which == 0 ? (const double *)ctx->dTgtU : (const double *)ctx->dV;
	const double *r = which == 0 ? (const double *)ctx->dTgtR : (const double *)ctx->dTgtCR;
	const double *qr = which == 0 ? (const double *)ctx->dTgtQr + 1 : (const double *)ctx->dV + Np + 1;
	const size_t ldu = which == 0 ? Np : ldv, ldq = which == 0 ? Rp : ldv;
	HIPCHK(ctx, hipMemcpy2DAsync(u_out, N * sizeof(double), u, ldu * sizeof(double), N * sizeof(double), (size_t)npoints, hipMemcpyDeviceToHost,
	                             ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(r_out, nreg * sizeof(double), r, Rp * sizeof(double), nreg * sizeof(double), (size_t)npoints,
	                             hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(qr_out, nreg * sizeof(double), qr, ldq * sizeof(double), nreg * sizeof(double), (size_t)npoints,
	                             hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// second order: pair covariances, their emulator uncertainty and the two-way surface (gpemu.h).  The tables
// and constants of gpemu_sens_cov, then the leave-two-out products, the pair sweep and its finish; everything written is the
// entries' own (dSensPrep, dSensCst, dSensPex2, dSensPairPart, dSensPairOut; the post entry also dSensP, dSensG).
// ---------------------------------------------------------------------------
static int sens_pair_check(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi, SensBox *bx)
{
	if (const int rc = sens_check(a, b, lo, hi, bx)) return rc;
	if (a->d < 2) return fail(a, GPEMU_ERR_ARG, "sensitivity: a pair needs two parameters");
	return GPEMU_OK;
}

// the tables of both contexts and their leave-two-out products
static int sens_pair_prep(gpemu_ctx *a, const SensBox &bx, int cls)
{
	const int N = a->N, d = a->d;
	if (const int rc = sens_prep(a, bx, cls)) return rc;
	// per point d (d - 1) / 2 values of two products each, once per context
	ProfScope ps(a, cls, 2.0 * N * d * (d - 1.0), 8.0 * 3.0 * (double)sens_pex2_elems(N, d));
	HIPCHK(a, launch_sens_pair_prep(a->stream, a->dSensPrep, N, d, a->dSensPex2));
	return GPEMU_OK;
}

extern "C" int gpemu_sens_pairs_dev(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi, double *out_dev)
{
	if (!a || !b || !lo || !hi || !out_dev) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_pair_check(a, b, lo, hi, &bx)) return rc;
	HIPCHK(a, hipSetDevice(a->device));
	const int N = a->N, d = a->d, Np = a->Np;
	const double npairs = d * (d - 1) / 2.0, nb = (d + 7) / 8, nii = 8.0 * nb + 8.0 * nb * (nb - 1.0);   // II values per pair of points
	int rc = grow(a, a->dSensPex2, sens_pex2_elems(N, d));
	if (!rc) rc = grow(a, a->dSensPairPart, sens_pair_part_elems(N, d));
	if (rc) return rc;
	if ((rc = sens_order_streams(a, b))) return rc;
	if (prof_on(a, GPEMU_PROF_SENS))
		for (const char *t : {"sens_prep", "sens_pair_prep", "sens_pair_sweep", "sens_pair_finish"}) a->prof.tag.push_back(t);
	if ((rc = sens_pair_prep(a, bx, GPEMU_PROF_SENS))) return rc;
	const double *gamA = a->dLinvAug + (size_t)Np * Np, *gamB = b->dLinvAug + (size_t)Np * Np;
	{
		// per pair of points: the II values of gpemu_sens_cov (19 flops each) for 8 coordinates per diagonal block and 16 per
		// other block, then 3 flops per pair of coordinates (both launches under one scope when d > 8)
		ProfScope ps(a, GPEMU_PROF_SENS, (double)N * N * (sens_pair_flops(bx, nii) + 3.0 * npairs), 8.0 * (double)sens_pair_part_elems(N, d));
		HIPCHK(a, launch_sens_pair_sweep(a->stream, a->dX, N, d, gamA, gamB, a->dSensPex2, a->dSensCst, bx.meas, nullptr, a->dSensPairPart));
	}
	{
		ProfScope ps(a, GPEMU_PROF_SENS, (double)sens_pair_part_elems(N, d), 8.0 * (double)sens_pair_part_elems(N, d));
		HIPCHK(a, launch_sens_pair_finish(a->stream, a->dSensPairPart, N, d, a->order, gamA, a->dBetaQ, a->pred_cov.amp, gamB, b->dBetaQ,
		                                  b->pred_cov.amp, a->dSensPrep, a->dSensCst, out_dev));
	}
	if (a != b) {
		// b's later work (a new set-up would rewrite its gamma) runs behind this call
		HIPCHK(a, hipEventRecord(a->sens_ev2, a->stream));
		HIPCHK(a, hipStreamWaitEvent(b->stream, a->sens_ev2, 0));
	}
	return GPEMU_OK;
}

extern "C" int gpemu_sens_pairs(gpemu_ctx *a, gpemu_ctx *b, const double *lo, const double *hi, double *cov_pair)
{
	if (!a || !b || !lo || !hi || !cov_pair) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_pair_check(a, b, lo, hi, &bx)) return rc;
	HIPCHK(a, hipSetDevice(a->device));
	const size_t npairs = (size_t)a->d * (a->d - 1) / 2;
	if (const int rc = grow(a, a->dSensPairOut, npairs)) return rc;
	if (const int rc = gpemu_sens_pairs_dev(a, b, lo, hi, a->dSensPairOut)) return rc;
	HIPCHK(a, hipMemcpyAsync(cov_pair, a->dSensPairOut, npairs * sizeof(double), hipMemcpyDeviceToHost, a->stream));
	HIPCHK(a, hipStreamSynchronize(a->stream));
	return GPEMU_OK;
}

extern "C" int gpemu_sens_pairs_post_dev(gpemu_ctx *ctx, const double *lo, const double *hi, double *out_dev)
{
	if (!ctx || !lo || !hi || !out_dev) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_pair_check(ctx, ctx, lo, hi, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int N = ctx->N, d = ctx->d, nreg = ctx->nreg, Rp = ctx->Rp;
	const size_t ldp = (size_t)round_up(N, 64);
	const double ntl = (double)(ldp / 64) * (double)(ldp / 64 + 1) / 2.0;           // lower tiles
	const double npairs = d * (d - 1) / 2.0, nb = (d + 7) / 8, nii = 8.0 * nb + 8.0 * nb * (nb - 1.0);   // II values per pair of points
	int rc = grow(ctx, ctx->dSensPex2, sens_pex2_elems(N, d));
	if (!rc) rc = grow(ctx, ctx->dSensPairPart, sens_pair_part_elems(N, d));
	if (!rc) rc = grow(ctx, ctx->dSensP, ldp * ldp);
	if (!rc) rc = grow(ctx, ctx->dSensG, (size_t)N * nreg);
	if (rc) return rc;
	if (prof_on(ctx, GPEMU_PROF_SENS_POST))
		for (const char *t : {"sens_prep", "sens_pair_prep", "sens_pmat", "sens_pair_sweep_weighted", "sens_pair_post_finish"})
			ctx->prof.tag.push_back(t);
	if ((rc = sens_pair_prep(ctx, bx, GPEMU_PROF_SENS_POST))) return rc;
	if ((rc = ensure_corner(ctx))) return rc;
	const double *Q = ctx->dBetaQ + nreg;
	{
		ProfScope ps(ctx, GPEMU_PROF_SENS_POST, ntl * (128.0 * nreg * nreg + 4096.0 * (2.0 * nreg + 1.0)), 8.0 * ntl * 8192.0);
		HIPCHK(ctx, launch_sens_pmat(ctx->stream, ctx->dS, (long)ctx->S_dim, Rp, Q, N, nreg, ctx->dSensG, ctx->dSensP));
	}
	{
		ProfScope ps(ctx, GPEMU_PROF_SENS_POST, ntl * 4096.0 * (sens_pair_flops(bx, nii) + nii + 3.0 * npairs),
		             8.0 * ntl * (4096.0 * nb * (nb + 1.0) / 2.0 + npairs));
		HIPCHK(ctx, launch_sens_pair_sweep(ctx->stream, ctx->dX, N, d, nullptr, nullptr, ctx->dSensPex2, ctx->dSensCst, bx.meas, ctx->dSensP,
		                                   ctx->dSensPairPart));
	}
	{
		ProfScope ps(ctx, GPEMU_PROF_SENS_POST, ntl * npairs + npairs * nreg * (2.0 * nreg + 4.0 * N),
		             8.0 * (ntl * npairs + npairs * 3.0 * N * nreg));
		HIPCHK(ctx, launch_sens_pair_post_finish(ctx->stream, ctx->dSensPairPart, N, d, nreg, ctx->pred_cov.amp, ctx->dSensPrep, ctx->dSensCst,
		                                         ctx->dSensG, Q, out_dev));
	}
	ctx->sens_post_N = N;
	return GPEMU_OK;
}

extern "C" int gpemu_sens_pairs_post(gpemu_ctx *ctx, const double *lo, const double *hi, double *s_pair)
{
	if (!ctx || !lo || !hi || !s_pair) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_pair_check(ctx, ctx, lo, hi, &bx)) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t npairs = (size_t)ctx->d * (ctx->d - 1) / 2;
	if (const int rc = grow(ctx, ctx->dSensPairOut, npairs)) return rc;
	if (const int rc = gpemu_sens_pairs_post_dev(ctx, lo, hi, ctx->dSensPairOut)) return rc;
	HIPCHK(ctx, hipMemcpyAsync(s_pair, ctx->dSensPairOut, npairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

extern "C" int gpemu_sens_joint(gpemu_ctx *ctx, const double *lo, const double *hi, int j, int k, int npts, const double *xj,
                                const double *xk, double *e0, double *joint, double *inter)
{
	if (!ctx || !lo || !hi || !xj || !xk || !e0 || !joint) return GPEMU_ERR_ARG;
	SensBox bx;
	if (const int rc = sens_pair_check(ctx, ctx, lo, hi, &bx)) return rc;
	const int N = ctx->N, d = ctx->d, Np = ctx->Np;
	if (j == k || j < 0 || k < 0 || j >= d || k >= d) return fail(ctx, GPEMU_ERR_ARG, "sensitivity: a pair is two different parameters of 0 .. d - 1");
	if (npts < 1) return fail(ctx, GPEMU_ERR_ARG, "sensitivity: npts < 1");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t ng = (size_t)npts;
	int rc = grow(ctx, ctx->dSensGrid, 4 * ng);
	if (!rc) rc = grow(ctx, ctx->dSensOut, 3 + 2 * (size_t)GPEMU_MAX_PARAMS);
	if (!rc) rc = grow(ctx, ctx->dSensPex2, sens_pex2_elems(N, d));
	if (rc) return rc;
	// the smaller coordinate first: the tables are numbered by j < k
	double *dxj = ctx->dSensGrid, *dxk = dxj + ng, *djoint = dxk + ng, *dinter = djoint + ng;
	HIPCHK(ctx, hipMemcpyAsync(j < k ? dxj : dxk, xj, ng * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(j < k ? dxk : dxj, xk, ng * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (prof_on(ctx, GPEMU_PROF_SENS)) for (const char *t : {"sens_prep", "sens_pair_prep", "sens_joint"}) ctx->prof.tag.push_back(t);
	if ((rc = sens_pair_prep(ctx, bx, GPEMU_PROF_SENS))) return rc;
	{
		ProfScope ps(ctx, GPEMU_PROF_SENS, (double)ng * N * 16.0, 8.0 * 4.0 * (double)ng);
		HIPCHK(ctx, launch_sens_joint(ctx->stream, ctx->dX, N, d, ctx->order, ctx->dLinvAug + (size_t)Np * Np, ctx->dBetaQ, ctx->pred_cov.amp,
		                              ctx->dSensPrep, ctx->dSensPex2, ctx->dSensCst, std::min(j, k), std::max(j, k), npts, dxj, dxk,
		                              ctx->dSensOut, djoint, dinter));
	}
	HIPCHK(ctx, hipMemcpyAsync(joint, djoint, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (inter) HIPCHK(ctx, hipMemcpyAsync(inter, dinter, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(e0, ctx->dSensOut, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// gradient (gradFnMulti, maxmultimin.c:416-550) and value+gradient (evalFnGradMulti, :615-618)
//
// One implementation for one evaluation and for a lock-step batch, in two halves:
//   enqueue: stage nb matrices with their inverse rows, factor them in lock-step (U = L^-T falls out), Gram / log det
//            as for a likelihood batch; then per chunk of corners C^-1 = U U^T (one batched GEMM), alpha = C^-1 y (or
//            C^-1 (y - H beta) with beta solved on the device, exact mode), the tile reductions tr(C^-1 dC_k),
//            alpha^T dC_k alpha, their second-stage sums, and one small copy into the pinned result ring.  No host
//            synchronisation anywhere: the call returns while the device works.
//   collect: waits for THAT batch's event and finishes on the host (nreg x nreg solve, the reference's scalings).
// ---------------------------------------------------------------------------
// corners S kept in flight at a time by the gradient of a batch: as many as fit in about 10 GB
static int grad_chunk_size(const gpemu_ctx *ctx, int nb)
{
	const double dim = (double)ctx->Np + ctx->Rp;
	const int fit = (int)(10.0e9 / (dim * dim * 8.0));
	return std::max(1, std::min(nb, fit));
}

static int grad_check_args(gpemu_ctx *ctx, int nthetas)
{
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	const int trainable_matern = (ctx->mode & GPEMU_MODE_EXACT_GRAD) && (ctx->mode & GPEMU_MODE_MATERN_LOG);
	if (ctx->kind != GPEMU_POWEREXP && !trainable_matern)
		return fail(ctx, GPEMU_ERR_ARG,
		            "Matern gradient needs GPEMU_MODE_EXACT_GRAD | GPEMU_MODE_MATERN_LOG: the reference's literal Matern "
		            "derivative matrices (emulator.c:401-433, 497-532) carry an accumulator across elements and its training "
		            "path zeroes the raw amplitude (maxmultimin.c:311,495) -- there is no literal Matern gradient to reproduce");
	if (nthetas < nthetas_for(ctx)) return fail(ctx, GPEMU_ERR_ARG, "nthetas too small");
	if (nthetas > GPEMU_MAX_PARAMS + 2) return fail(ctx, GPEMU_ERR_ARG, "nthetas too large");
	return GPEMU_OK;
}

// What the gradient reductions of a chunk of corners work on besides the model: a view, no owner.  Production points it at
// the context's buffers (grad_enqueue_chunk), gpemu_test_grad_sums at buffers of its own.
struct GradWork {
	const double *S;        // nbc corners of side and leading dimension Np + Rp, one after the other
	double *ag;             // nbc slots of Np + 2 GPEMU_MAX_PARAMS doubles: alpha scratch | length thetas | beta
	double *part;           // nbc x ntiles x (2d + 2) tile sums
	double *sums;           // nbc rows of second-stage sums,
	long sums_stride;       //   this far apart
	const double *res;      // exact form: the Gram matrices of the elements (Rp x Rp, as finish_kernel leaves them),
	long rstride;           //   this far apart
	const CovParams *pp;    // device: the nbc elements' hyper-parameters
	double *gph;            // host staging of the length thetas, nbc x GPEMU_MAX_PARAMS: read by an asynchronous copy
	hipEvent_t gph_ev;      // recorded behind that copy (nullptr: none)
	bool exact;             // GPEMU_MODE_EXACT_GRAD form
	bool gram;              // exact form: the tile distances from the matrix unit (needs the centred design)
	int clamp;              // literal form: -1 = the rule below, 1 / 0 = grad_part_kernel<true> / <false> whatever it says
};

// literal form: exp(-1/2 e^{-2 theta_k} D_k^2) of every pair of design points -- when the largest such argument of the
// chunk stays small (|D_k| <= the coordinate's range) the kernel's exp needs no lower clamp
static bool grad_lit_noclamp(const gpemu_ctx *ctx, int nbc, const double *th, int nthetas)
{
	const int d = ctx->d, nlen = ctx->kind == GPEMU_POWEREXP ? d : 1;
	bool noclamp = (int)ctx->xhalf.size() == d;
	for (int i = 0; noclamp && i < nbc; i++)
		for (int k = 0; k < nlen; k++) {
			const double range = 2.0 * ctx->xhalf[k];
			if (!(0.5 * exp(-2.0 * th[(size_t)i * nthetas + 2 + k]) * range * range < 600.0)) noclamp = false;
		}
	return noclamp;
}

// everything of a chunk's gradient behind its corners, on the context's stream: the length thetas into the ag slots, beta
// on the device (exact form), alpha, the tile sums and their second-stage sums.  th: the chunk's first theta vector.
static int grad_sums_of_corners(gpemu_ctx *ctx, const GradWork &w, int nbc, const double *th, int nthetas)
{
	const int N = ctx->N, d = ctx->d, Rp = ctx->Rp;
	const size_t dim = (size_t)ctx->Np + Rp, sstride = dim * dim;
	const int nlen = ctx->kind == GPEMU_POWEREXP ? d : 1;           // length-scale directions
	const size_t gslot = (size_t)ctx->Np + 2 * GPEMU_MAX_PARAMS;
	const int nt = (N + 63) / 64, ntiles = nt * (nt + 1) / 2;
	const int np = 2 * d + 2;
	const size_t need = (size_t)ntiles * np;
	for (int i = 0; i < nbc; i++)
		for (int k = 0; k < GPEMU_MAX_PARAMS; k++)
			w.gph[(size_t)i * GPEMU_MAX_PARAMS + k] = k < nlen ? th[(size_t)i * nthetas + 2 + k] : 0.0;
	HIPCHK(ctx, hipMemcpy2DAsync(w.ag + ctx->Np, gslot * sizeof(double), w.gph, GPEMU_MAX_PARAMS * sizeof(double),
	                             GPEMU_MAX_PARAMS * sizeof(double), nbc, hipMemcpyHostToDevice, ctx->stream));
	if (w.gph_ev) HIPCHK(ctx, hipEventRecord(w.gph_ev, ctx->stream));
	if (w.exact)
		HIPCHK(ctx, launch_beta_solve(ctx->stream, w.res, w.rstride, Rp, ctx->nreg, nbc, w.ag, (long)gslot, ctx->Np));
	int nparts = 0;
	const bool noclamp = !w.exact && (w.clamp < 0 ? grad_lit_noclamp(ctx, nbc, th, nthetas) : w.clamp == 0);
	HIPCHK(ctx, launch_grad_partials(ctx->stream, w.S, (long)dim, Rp, (long)sstride, nbc, ctx->dX, N, d, w.ag, ctx->Np,
	                                 (long)gslot, w.part, (long)need, &nparts, w.exact ? ctx->kind : 0, ctx->nreg,
	                                 w.pp, noclamp, w.gram ? ctx->dXg : nullptr));
	HIPCHK(ctx, launch_grad_reduce(ctx->stream, w.part, (long)need, nparts, np, nbc, w.sums, w.sums_stride));
	return GPEMU_OK;
}

// gradient reductions of the batch elements b0 .. b0+nbc-1 of the factorisation in the workspace, into dGradSum
static int grad_enqueue_chunk(gpemu_ctx *ctx, int b0, int nbc, const double *th_all, int nthetas)
{
	const int N = ctx->N, d = ctx->d, Rp = ctx->Rp;
	const size_t dim = (size_t)ctx->Np + Rp, sstride = dim * dim;
	int rc = grow(ctx, ctx->dS, (size_t)nbc * sstride);
	if (rc) return rc;
	ctx->S_dim = dim;
	HIPCHK(ctx, build_corner(ctx, tall_of(ctx), ctx->dS, (long)dim, b0, nbc));
	const size_t gslot = (size_t)ctx->Np + 2 * GPEMU_MAX_PARAMS;    // per corner: alpha scratch | length thetas | beta
	rc = grow(ctx, ctx->dAlpha, (size_t)nbc * gslot);
	if (rc) return rc;
	const int nt = (N + 63) / 64, ntiles = nt * (nt + 1) / 2;
	rc = grow(ctx, ctx->dGradPart, (size_t)ntiles * (2 * d + 2) * nbc);
	if (rc) return rc;
	GradWork w{};
	w.S = ctx->dS; w.ag = ctx->dAlpha; w.part = ctx->dGradPart;
	w.sums = ctx->dGradSum + (size_t)b0 * gpemu_ctx::GRAD_NP_MAX; w.sums_stride = (long)gpemu_ctx::GRAD_NP_MAX;
	w.res = ctx->dRes + (size_t)b0 * ctx->res_len; w.rstride = (long)ctx->res_len;
	w.pp = ctx->dParams + b0;
	// the length thetas of the chunk: through the pinned entry that belongs to this batch's hyper-parameter upload (reused
	// only after the entry's event, re-recorded behind the copy out of it)
	w.gph = ctx->pring.gph + ((size_t)ctx->pring.slot * GPEMU_MAX_BATCH + b0) * GPEMU_MAX_PARAMS;
	w.gph_ev = ctx->pring.ev[ctx->pring.slot];
	w.exact = (ctx->mode & GPEMU_MODE_EXACT_GRAD) != 0;
	w.gram = ctx->sched.grad_gram != 0;
	w.clamp = -1;
	return grad_sums_of_corners(ctx, w, nbc, th_all + (size_t)b0 * nthetas, nthetas);
}

extern "C" int gpemu_loglik_grad_batch_enqueue(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas)
{
	if (!ctx || !thetas) return GPEMU_ERR_ARG;
	int rc = grad_check_args(ctx, nthetas);
	if (rc) return rc;
	if (nb < 1 || nb > GPEMU_MAX_BATCH) return fail(ctx, GPEMU_ERR_ARG, "batch size must be 1..GPEMU_MAX_BATCH");
	std::vector<double> th(thetas, thetas + (size_t)nb * nthetas);
	for (int b = 0; b < nb; b++) th[(size_t)b * nthetas] = 0.0;     // maxmultimin.c:441
	std::vector<CovParams> ps;
	rc = make_cov_params_batch(ctx, nb, th.data(), nthetas, &ps);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	invalidate_prediction(ctx);
	rc = stage_matrices(ctx, ps.data(), nb, 1);
	if (rc) return rc;
	rc = run_potrf(ctx, 1);
	if (rc) return rc;
	rc = enqueue_results(ctx);                       // Gram, log det, info words -> the next slot of the pinned ring
	if (rc) return rc;
	ResSlot &s = ctx->newest();
	// the ring entry becomes a collectable value+gradient batch only once EVERYTHING of it is on the stream: until then it
	// is marked empty (nb = 0), so that after a failure below a later collect of this slot is refused
	// (GPEMU_ERR_STATE) instead of returning a gradient built from whatever the pinned ring held
	s.nb = 0;
	s.kind = 1;
	s.th = th;
	s.nthetas = nthetas;
	s.mode = ctx->mode;
	const int chunk = grad_chunk_size(ctx, nb);
	for (int b0 = 0; b0 < nb; b0 += chunk) {
		rc = grad_enqueue_chunk(ctx, b0, std::min(chunk, nb - b0), th.data(), nthetas);
		if (rc) return rc;
	}
	HIPCHK(ctx, hipMemcpyAsync(s.grad, ctx->dGradSum, (size_t)nb * gpemu_ctx::GRAD_NP_MAX * sizeof(double), hipMemcpyDeviceToHost,
	                           ctx->stream));
	HIPCHK(ctx, hipEventRecord(s.ev, ctx->stream));                  // (re-recorded: now behind the gradient sums as well)
	s.nb = nb;
	return GPEMU_OK;
}

// host half of a value+gradient batch whose results sit in ring slot s (its event has been waited for)
static int grad_collect_slot(gpemu_ctx *ctx, const ResSlot &s, int nb, double *neg_loglik, double *sigma2, double *beta, double *grad,
                             int *info, int *status)
{
	const int nthetas = s.nthetas, ng = nthetas - 1, d = ctx->d;
	const bool exact = (s.mode & GPEMU_MODE_EXACT_GRAD) != 0;                     // as it was when the batch was enqueued
	const int nlen = ctx->kind == GPEMU_POWEREXP ? d : 1;
	for (int b = 0; b < nb; b++) {
		HostLik r;
		const int st = element_likelihood(ctx, s, b, info ? info + b : nullptr, &r);
		const bool ok = st == GPEMU_OK;                   // (any failure, the regression's too, leaves NaN everywhere)
		if (status) status[b] = st;
		if (neg_loglik) neg_loglik[b] = ok ? neg_loglik_of(r, ctx->N) : NAN;
		if (sigma2) sigma2[b] = ok ? r.sigma2 : NAN;
		if (beta) for (int a = 0; a < ctx->nreg; a++) beta[(size_t)b * ctx->nreg + a] = ok ? r.beta[a] : NAN;
		if (grad) for (int i = 0; i < ng; i++) grad[(size_t)b * ng + i] = NAN;
		if (!grad || !ok) continue;
		const double *sums = s.grad + (size_t)b * gpemu_ctx::GRAD_NP_MAX;
		double *g = grad + (size_t)b * ng;
		if (exact) {
			// d(-logL)/dtheta = 1/2 sum_ab (A_ab - alpha_a alpha_b) dC_ab: slot nlen = nugget direction, slots < nlen the lengths
			g[0] = 0.5 * sums[nlen];
			for (int k = 0; k < nlen; k++) g[k + 1] = 0.5 * sums[k];
		} else {
			const double aa = sums[2 * d + 1];
			const double amp = exp(log(r.sigma2));                          // maxmultimin.c:503,514
			const double nug = exp(s.th[(size_t)b * nthetas + 1]);           // :515
			// G(dC) = -1/2 tr(A dC) + 1/2 alpha^T dC alpha ;  grad = -G   (:527,535; getGradientCn :571-608)
			g[0] = -1.0 * (-0.5 * nug * sums[2 * d] + 0.5 * nug * aa);
			for (int k = 0; k < d; k++) g[k + 1] = -1.0 * (amp * (-0.5 * sums[2 * k] + 0.5 * sums[2 * k + 1]));
		}
	}
	return GPEMU_OK;
}

// results of the value+gradient batch enqueued `back` batches (of either kind) before the newest one; waits for it only
extern "C" int gpemu_loglik_grad_batch_collect_back(gpemu_ctx *ctx, int back, int nb, double *neg_loglik, double *sigma2,
                                                    double *beta, double *grad, int *info, int *status)
{
	if (!ctx) return GPEMU_ERR_ARG;
	const ResSlot *s = ring_slot_back(ctx, back, nb, 1);
	if (!s) return GPEMU_ERR_STATE;
	HIPCHK(ctx, hipEventSynchronize(s->ev));
	return grad_collect_slot(ctx, *s, nb, neg_loglik, sigma2, beta, grad, info, status);
}

extern "C" int gpemu_loglik_grad_batch_collect(gpemu_ctx *ctx, int nb, double *neg_loglik, double *sigma2, double *beta,
                                               double *grad, int *info, int *status)
{
	return gpemu_loglik_grad_batch_collect_back(ctx, 0, nb, neg_loglik, sigma2, beta, grad, info, status);
}

// evalFnGradMulti for a list of thetas (the line-search points of independent restarts): enqueue + collect
extern "C" int gpemu_loglik_grad_batch(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas, double *neg_loglik,
                                       double *sigma2, double *beta, double *grad, int *info, int *status)
{
	if (!ctx || !grad || !thetas) return GPEMU_ERR_ARG;
	int rc = gpemu_loglik_grad_batch_enqueue(ctx, nb, thetas, nthetas);
	if (rc) return rc;
	return gpemu_loglik_grad_batch_collect(ctx, nb, neg_loglik, sigma2, beta, grad, info, status);
}

// evalFnGradMulti (maxmultimin.c:615-618) with ONE factorisation shared by value and gradient: a batch of one
extern "C" int gpemu_loglik_grad(gpemu_ctx *ctx, const double *thetas, int nthetas, double *neg_loglik, double *sigma2,
                                 double *beta, double *grad, int *info)
{
	if (!ctx || !grad) return GPEMU_ERR_ARG;
	int st = GPEMU_OK;
	int rc = gpemu_loglik_grad_batch(ctx, 1, thetas, nthetas, neg_loglik, sigma2, beta, grad, info, &st);
	return rc ? rc : st;
}

extern "C" int gpemu_grad(gpemu_ctx *ctx, const double *thetas, int nthetas, double *grad, int *info)
{
	return gpemu_loglik_grad(ctx, thetas, nthetas, nullptr, nullptr, nullptr, grad, info);
}

// ---------------------------------------------------------------------------
// implausibility and calibration likelihood against observations (gpemu.h).  The set-up is host arithmetic
// (gpemu_calib_project, kernels_calib.hip) and one upload of the table; an evaluation is one launch, a selection three, the
// gradient of chi2 and logpdf one.
// ---------------------------------------------------------------------------
extern "C" int gpemu_calib_setup(gpemu_ctx *ctx, int nt, int nr, const double *ybar, const double *A, const double *z, const double *S,
                                 const double *sd, const double *rel, int *info)
{
	if (info) *info = 0;
	if (!ctx || !info) return GPEMU_ERR_ARG;
	if (rel && nt >= 1 && nt <= GPEMU_CALIB_MAX_NT)
		for (int t = 0; t < nt; t++)
			if (!(rel[t] >= 0.0) || !std::isfinite(rel[t])) return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_setup: rel must be finite and >= 0");
	if (nt < 1 || nr < 1) return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_setup: bad argument");
	std::vector<double> mhat(GPEMU_CALIB_MAX_R), sigz(GPEMU_CALIB_MAX_R * GPEMU_CALIB_MAX_R);
	double consts[3];
	const int rc = gpemu_calib_project(nt, nr, ybar, A, z, S, sd, mhat.data(), sigz.data(), consts, info);
	if (rc == GPEMU_ERR_NOT_PD) return fail(ctx, rc, "gpemu_calib_setup: S or A^T S^-1 A is not positive definite");
	if (rc) return fail(ctx, rc, "gpemu_calib_setup: bad argument (NULL pointer, size beyond the limits, non-finite input, sd <= 0)");
	std::vector<double> sdiag(nt), tab(calib_table_elems(nt, nr));
	for (int t = 0; t < nt; t++) sdiag[t] = S ? S[(size_t)t * nt + t] : sd[t] * sd[t];
	calib_fill_table(nt, nr, ybar, A, z, sdiag.data(), rel, mhat.data(), sigz.data(), consts, tab.data());
	HIPCHK(ctx, hipSetDevice(ctx->device));
	// work enqueued against the old table ends before the new one replaces it (the upload below reads pageable memory: it
	// has completed when the call returns)
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->calib_nt = 0;
	const int gr = grow(ctx, ctx->dCalibTab, tab.size());
	if (gr) return gr;
	HIPCHK(ctx, hipMemcpyAsync(ctx->dCalibTab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->calib_nt = nt; ctx->calib_nr = nr;
	return GPEMU_OK;
}

extern "C" int gpemu_calib_release(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->calib_nt = ctx->calib_nr = 0;
	ctx->dCalibTab.reset(); ctx->dCalibIO.reset();
	ctx->dCalibIdx.reset(); ctx->dCalibCnt.reset();
	ctx->hCalibCnt.reset();
	return GPEMU_OK;
}

extern "C" int gpemu_calib_eval_dev(gpemu_ctx *ctx, int M, const double *mean_dev, const double *var_dev, int ld, double *stat_dev,
                                    int *worst_dev)
{
	if (!ctx || !mean_dev || !var_dev || !stat_dev || !worst_dev || M < 1 || ld < M) return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_eval: bad argument");
	if (!ctx->calib_nt) return fail(ctx, GPEMU_ERR_STATE, "gpemu_calib_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const double nt = ctx->calib_nt, nr = ctx->calib_nr, R = calib_pad(ctx->calib_nr);
	if (prof_on(ctx, GPEMU_PROF_CALIB)) ctx->prof.tag.push_back("calib_eval");
	ProfScope ps(ctx, GPEMU_PROF_CALIB, (double)M * (4.0 * nt * R + 8.0 * nt + R * R * R / 3.0 + 2.0 * R * R),
	             8.0 * M * (2.0 * nr + 5.0) + 4.0 * M);
	HIPCHK(ctx, launch_calib_eval(ctx->stream, ctx->dCalibTab, ctx->calib_nt, ctx->calib_nr, M, mean_dev, var_dev, ld, stat_dev, worst_dev));
	return GPEMU_OK;
}

extern "C" int gpemu_calib_eval(gpemu_ctx *ctx, int M, const double *mean, const double *var, int ld, double *stat, int *worst)
{
	if (!ctx || !mean || !var || !stat || !worst || M < 1 || ld < M) return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_eval: bad argument");
	if (!ctx->calib_nt) return fail(ctx, GPEMU_ERR_STATE, "gpemu_calib_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t nr = (size_t)ctx->calib_nr, m = (size_t)M, in = nr * m;     // the device copies are packed: leading dimension M
	int rc = grow(ctx, ctx->dCalibIO, 2 * in + 5 * m);
	if (!rc) rc = grow(ctx, ctx->dCalibIdx, m);
	if (rc) return rc;
	double *dm = ctx->dCalibIO, *dv = dm + in, *ds = dv + in;
	HIPCHK(ctx, hipMemcpy2DAsync(dm, m * sizeof(double), mean, (size_t)ld * sizeof(double), m * sizeof(double), nr, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(dv, m * sizeof(double), var, (size_t)ld * sizeof(double), m * sizeof(double), nr, hipMemcpyHostToDevice, ctx->stream));
	rc = gpemu_calib_eval_dev(ctx, M, dm, dv, M, ds, ctx->dCalibIdx);
	if (rc) return rc;
	HIPCHK(ctx, hipMemcpyAsync(stat, ds, 5 * m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(worst, ctx->dCalibIdx, m * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// gradients of chi2 and logpdf with respect to the query coordinates: one launch
extern "C" int gpemu_calib_grad_dev(gpemu_ctx *ctx, int M, int d, const double *mean_dev, const double *var_dev, int ld,
                                    const double *gmean_dev, const double *gvar_dev, long ldg, double *gchi2_dev, double *glogpdf_dev)
{
	if (!ctx || !mean_dev || !var_dev || !gmean_dev || !gvar_dev || (!gchi2_dev && !glogpdf_dev) || M < 1 || d < 1 || ld < M ||
	    ldg < (long)M * d)
		return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_grad: bad argument");
	if (!ctx->calib_nt) return fail(ctx, GPEMU_ERR_STATE, "gpemu_calib_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const double nr = ctx->calib_nr, R = calib_pad(ctx->calib_nr);
	if (prof_on(ctx, GPEMU_PROF_CALIB)) ctx->prof.tag.push_back("calib_grad");
	ProfScope ps(ctx, GPEMU_PROF_CALIB, (double)M * (R * R * R / 2.0 + 3.0 * R * R + 8.0 * nr * d),
	             8.0 * M * (2.0 * nr + 2.0 * nr * d + (gchi2_dev ? d : 0) + (glogpdf_dev ? d : 0)));
	HIPCHK(ctx, launch_calib_grad(ctx->stream, ctx->dCalibTab, ctx->calib_nr, M, d, mean_dev, var_dev, ld, gmean_dev, gvar_dev, ldg,
	                              gchi2_dev, glogpdf_dev));
	return GPEMU_OK;
}

extern "C" int gpemu_calib_grad(gpemu_ctx *ctx, int M, int d, const double *mean, const double *var, int ld, const double *gmean,
                                const double *gvar, long ldg, double *gchi2, double *glogpdf)
{
	if (!ctx || !mean || !var || !gmean || !gvar || (!gchi2 && !glogpdf) || M < 1 || d < 1 || ld < M || ldg < (long)M * d)
		return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_grad: bad argument");
	if (!ctx->calib_nt) return fail(ctx, GPEMU_ERR_STATE, "gpemu_calib_setup has not been called");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	// the device copies are packed: leading dimensions M and M * d
	const size_t nr = (size_t)ctx->calib_nr, m = (size_t)M, in = nr * m, md = m * (size_t)d, gin = nr * md;
	int rc = grow(ctx, ctx->dCalibIO, 2 * in + 2 * gin + 2 * md);
	if (rc) return rc;
	double *dm = ctx->dCalibIO, *dv = dm + in, *dgm = dv + in, *dgv = dgm + gin, *dc = dgv + gin, *dl = dc + md;
	const size_t w = m * sizeof(double), wg = md * sizeof(double);
	HIPCHK(ctx, hipMemcpy2DAsync(dm, w, mean, (size_t)ld * sizeof(double), w, nr, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(dv, w, var, (size_t)ld * sizeof(double), w, nr, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(dgm, wg, gmean, (size_t)ldg * sizeof(double), wg, nr, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(dgv, wg, gvar, (size_t)ldg * sizeof(double), wg, nr, hipMemcpyHostToDevice, ctx->stream));
	rc = gpemu_calib_grad_dev(ctx, M, d, dm, dv, M, dgm, dgv, (long)md, gchi2 ? dc : nullptr, glogpdf ? dl : nullptr);
	if (rc) return rc;
	if (gchi2) HIPCHK(ctx, hipMemcpyAsync(gchi2, dc, wg, hipMemcpyDeviceToHost, ctx->stream));
	if (glogpdf) HIPCHK(ctx, hipMemcpyAsync(glogpdf, dl, wg, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

extern "C" int gpemu_calib_select_dev(gpemu_ctx *ctx, int M, const double *stat_dev, double cut_chi2, int level, double cut_I, int *idx_dev,
                                      int *count)
{
	if (count) *count = 0;
	if (!ctx || !stat_dev || !idx_dev || !count || M < 1 || level < 1 || level > 3 || cut_chi2 != cut_chi2 || cut_I != cut_I)
		return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_select: bad argument");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int nb = calib_select_blocks(M);
	int rc = grow(ctx, ctx->dCalibCnt, (size_t)nb + 1);
	if (!rc) rc = grow(ctx, ctx->hCalibCnt, 1);
	if (rc) return rc;
	{
		if (prof_on(ctx, GPEMU_PROF_CALIB)) ctx->prof.tag.push_back("calib_select");
		ProfScope ps(ctx, GPEMU_PROF_CALIB, 0.0, 36.0 * M + 8.0 * nb);
		HIPCHK(ctx, launch_calib_select(ctx->stream, stat_dev, M, cut_chi2, level, cut_I, ctx->dCalibCnt, idx_dev));
	}
	HIPCHK(ctx, hipMemcpyAsync(ctx->hCalibCnt, ctx->dCalibCnt + nb, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	*count = ctx->hCalibCnt[0];
	return GPEMU_OK;
}

extern "C" int gpemu_calib_gather_dev(gpemu_ctx *ctx, int M, const double *stat_dev, const int *worst_dev, int count, const int *idx_dev,
                                      double *out_dev, int *worst_out_dev)
{
	if (!ctx || !stat_dev || !idx_dev || !out_dev || M < 1 || count < 0) return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_gather: bad argument");
	if (!count) return GPEMU_OK;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_calib_gather(ctx->stream, stat_dev, worst_dev, M, count, idx_dev, out_dev, worst_dev ? worst_out_dev : nullptr));
	return GPEMU_OK;
}

extern "C" int gpemu_calib_select(gpemu_ctx *ctx, int M, const double *stat, double cut_chi2, int level, double cut_I, int *idx, int *count)
{
	if (count) *count = 0;
	if (!ctx || !stat || !idx || !count || M < 1 || level < 1 || level > 3 || cut_chi2 != cut_chi2 || cut_I != cut_I)
		return fail(ctx, GPEMU_ERR_ARG, "gpemu_calib_select: bad argument");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t m = (size_t)M;
	int rc = grow(ctx, ctx->dCalibIO, 5 * m);
	if (!rc) rc = grow(ctx, ctx->dCalibIdx, m);
	if (rc) return rc;
	// the two rows the cuts read: chi2 and the level-th largest implausibility, at their places in a 5 x M layout
	HIPCHK(ctx, hipMemcpyAsync(ctx->dCalibIO, stat, m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(ctx->dCalibIO + (size_t)(1 + level) * m, stat + (size_t)(1 + level) * m, m * sizeof(double),
	                           hipMemcpyHostToDevice, ctx->stream));
	rc = gpemu_calib_select_dev(ctx, M, ctx->dCalibIO, cut_chi2, level, cut_I, ctx->dCalibIdx, count);
	if (rc) return rc;
	if (*count > 0) {
		HIPCHK(ctx, hipMemcpyAsync(idx, ctx->dCalibIdx, (size_t)*count * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// posterior samples of the parameters: the affine-invariant ensemble sampler (gpemu.h).  The prior table and
// every buffer of a run belong to ctx->sample.  The primitives are one launch each on the context's stream; the run is their
// sequence with the prediction sweeps of the components on the components' own streams, ordered by events.
// ---------------------------------------------------------------------------
extern "C" int gpemu_sample_set_prior(gpemu_ctx *ctx, int d, const int *kind, const double *lo, const double *hi)
{
	if (!ctx || !lo || !hi || d < 1 || d > GPEMU_MAX_PARAMS) return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_set_prior: bad argument");
	for (int l = 0; l < d; l++) {
		const int k = kind ? kind[l] : GPEMU_MEASURE_UNIFORM;
		if (k != GPEMU_MEASURE_UNIFORM && k != GPEMU_MEASURE_GAUSS)
			return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_set_prior: a kind is GPEMU_MEASURE_UNIFORM or GPEMU_MEASURE_GAUSS");
		if (k == GPEMU_MEASURE_GAUSS) {
			if (!std::isfinite(lo[l]) || !std::isfinite(hi[l]) || !(hi[l] > 0.0))
				return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_set_prior: a Gaussian coordinate needs a finite mean and a finite standard deviation > 0");
		} else if (!std::isfinite(lo[l]) || !std::isfinite(hi[l]) || !(hi[l] > lo[l]) || !std::isfinite(hi[l] - lo[l]))
			return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_set_prior: every bound must be finite, with hi > lo");
	}
	double tab[SAMPLE_PRIOR_ROWS * GPEMU_MAX_PARAMS];
	sample_fill_prior(d, kind, lo, hi, tab);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	// work enqueued against the old table ends before the new one replaces it, and the upload has completed on return
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->sample.prior_d = 0;
	if (const int rc = grow(ctx, ctx->sample.prior, sizeof tab / sizeof tab[0])) return rc;
	HIPCHK(ctx, hipMemcpyAsync(ctx->sample.prior, tab, sizeof tab, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->sample.prior_d = d;
	return GPEMU_OK;
}

extern "C" int gpemu_sample_release(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	ctx->sample.release();
	return GPEMU_OK;
}

extern "C" int gpemu_test_sample_chunk(gpemu_ctx *ctx, int records)
{
	if (!ctx || records < 0) return GPEMU_ERR_ARG;
	ctx->sample.chunk_records = records;
	return GPEMU_OK;
}

// the checks the two primitives share
static int sample_step_check(gpemu_ctx *ctx, int W, int d, int half, const char *who)
{
	if (W < 2 || (W & 1) || d < 1 || d > GPEMU_MAX_PARAMS || (half != 0 && half != 1)) return fail(ctx, GPEMU_ERR_ARG, who);
	if (ctx->sample.prior_d != d) return fail(ctx, GPEMU_ERR_STATE, "gpemu_sample_set_prior has not been called for this d");
	return GPEMU_OK;
}

extern "C" int gpemu_sample_propose_dev(gpemu_ctx *ctx, int W, int d, int half, unsigned long long step, unsigned long long seed, double a,
                                        const double *x_dev, double *y_dev, double *aux_dev)
{
	if (!ctx || !x_dev || !y_dev || !aux_dev || !(a > 1.0) || !std::isfinite(a)) return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_propose: bad argument");
	if (const int rc = sample_step_check(ctx, W, d, half, "gpemu_sample_propose: bad argument")) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_sample_propose(ctx->stream, ctx->sample.prior, W, d, half, step, seed, a, x_dev, y_dev, aux_dev));
	return GPEMU_OK;
}

extern "C" int gpemu_sample_accept_dev(gpemu_ctx *ctx, int W, int d, int half, unsigned long long step, unsigned long long seed,
                                       const double *y_dev, const double *aux_dev, const double *loglik_dev, double *x_dev, double *lp_dev,
                                       int *naccept_dev)
{
	if (!ctx || !y_dev || !aux_dev || !loglik_dev || !x_dev || !lp_dev || !naccept_dev)
		return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_accept: bad argument");
	if (const int rc = sample_step_check(ctx, W, d, half, "gpemu_sample_accept: bad argument")) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_sample_accept(ctx->stream, W, d, half, step, seed, y_dev, aux_dev, loglik_dev, x_dev, lp_dev, naccept_dev));
	return GPEMU_OK;
}

extern "C" int gpemu_sample_logpost_dev(gpemu_ctx *ctx, int M, int d, const double *x_dev, const double *loglik_dev, double *lp_dev)
{
	if (!ctx || !x_dev || !loglik_dev || !lp_dev || M < 1 || d < 1 || d > GPEMU_MAX_PARAMS)
		return fail(ctx, GPEMU_ERR_ARG, "gpemu_sample_logpost: bad argument");
	if (ctx->sample.prior_d != d) return fail(ctx, GPEMU_ERR_STATE, "gpemu_sample_set_prior has not been called for this d");
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, launch_sample_logpost(ctx->stream, ctx->sample.prior, M, d, x_dev, loglik_dev, lp_dev));
	return GPEMU_OK;
}

// the trace records of a chunk unless the test hook says otherwise: 64 MiB of staged records, one at the least
constexpr size_t SAMPLE_CHUNK_BYTES = (size_t)64 << 20;

// the log likelihood of the h points at xq into row 1 of the state's stat: every component's sweep on its own stream behind
// the obs stream's pending work, the obs stream behind the sweeps, the evaluation.  Nothing waits on the host.
static int sample_loglik(gpemu_ctx *const *comp, int nr, gpemu_ctx *obs, int h, const double *xq)
{
	SampleState &st = obs->sample;
	HIPCHK(obs, hipEventRecord(st.ev_obs, obs->stream));
	for (int c = 0; c < nr; c++) {
		gpemu_ctx *cc = comp[c];
		if (cc != obs) HIPCHK(obs, hipStreamWaitEvent(cc->stream, st.ev_obs, 0));
		const int rc = gpemu_predict_batch_dev(cc, h, xq, st.mean + (size_t)c * h, st.var + (size_t)c * h);
		if (rc) return cc == obs ? rc : fail(obs, rc, gpemu_last_error(cc));
		if (cc != obs) {
			HIPCHK(obs, hipEventRecord(st.ev_comp[c], cc->stream));
			HIPCHK(obs, hipStreamWaitEvent(obs->stream, st.ev_comp[c], 0));
		}
	}
	return gpemu_calib_eval_dev(obs, h, st.mean, st.var, h, st.stat, st.worst);
}

extern "C" int gpemu_calib_sample(gpemu_ctx *const *comp, int nr, gpemu_ctx *obs, const gpemu_sample_args *args, const double *x0,
                                  double *trace_x, double *trace_lp, double *x_end, double *lp_end, int *naccept, int *nrec_out)
{
	if (nrec_out) *nrec_out = 0;
	if (!obs) return GPEMU_ERR_ARG;
	if (!comp || !args || !x0 || !x_end || !lp_end || !naccept || !nrec_out || nr < 1)
		return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: bad argument");
	for (int c = 0; c < nr; c++)
		if (!comp[c]) return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: bad argument");
	const int W = args->nwalkers, h = W / 2;
	if (W < 2 || (W & 1) || args->nsteps < 1 || args->burn < 0 || args->thin < 1 || !(args->a > 1.0) || !std::isfinite(args->a))
		return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: bad argument");
	for (int c = 0; c < nr; c++)
		if (!comp[c]->pred_ready) return fail(obs, GPEMU_ERR_STATE, "gpemu_calib_sample: a component has no prediction set-up");
	const int d = comp[0]->d;
	for (int c = 0; c < nr; c++) {
		if (comp[c]->device != obs->device) return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: the contexts are on different devices (not built)");
		if (comp[c]->d != d) return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: the components differ in d");
	}
	if (h < d + 1) return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: each half of the walkers needs at least d + 1 of them");
	if (!obs->calib_nt) return fail(obs, GPEMU_ERR_STATE, "gpemu_calib_setup has not been called");
	if (obs->calib_nr != nr) return fail(obs, GPEMU_ERR_STATE, "gpemu_calib_sample: the calibration set-up has another number of components");
	if (obs->sample.prior_d != d) return fail(obs, GPEMU_ERR_STATE, "gpemu_sample_set_prior has not been called for this d");
	HIPCHK(obs, hipSetDevice(obs->device));

	// which global steps are recorded: burn and thin count global steps
	const unsigned long long g0 = args->first_step, thin = (unsigned long long)args->thin, burn = (unsigned long long)args->burn;
	auto recorded = [&](unsigned long long g) { return g >= burn && (g + 1) % thin == 0; };
	int nrec = 0;
	for (int t = 0; t < args->nsteps; t++) nrec += recorded(g0 + (unsigned long long)t);
	const bool keep = (trace_x || trace_lp) && nrec > 0;
	const size_t wd = (size_t)W * d;
	size_t chunk = obs->sample.chunk_records > 0 ? (size_t)obs->sample.chunk_records
	                                             : std::max<size_t>(1, SAMPLE_CHUNK_BYTES / (sizeof(double) * (wd + W)));
	chunk = std::min(chunk, (size_t)std::max(nrec, 1));

	// the state: allocated once per call shape, nothing inside the step loop
	SampleState &st = obs->sample;
	int rc = grow(obs, st.x, wd);
	if (!rc) rc = grow(obs, st.lp, W);
	if (!rc) rc = grow(obs, st.nacc, W);
	if (!rc) rc = grow(obs, st.y, (size_t)h * d);
	if (!rc) rc = grow(obs, st.aux, W);
	if (!rc) rc = grow(obs, st.mean, (size_t)nr * h);
	if (!rc) rc = grow(obs, st.var, (size_t)nr * h);
	if (!rc) rc = grow(obs, st.stat, 5 * (size_t)h);
	if (!rc) rc = grow(obs, st.worst, h);
	if (!rc && keep) rc = grow(obs, st.trx, chunk * wd);
	if (!rc && keep) rc = grow(obs, st.trlp, chunk * W);
	if (rc) return rc;
	if (!st.ev_obs) HIPCHK(obs, hipEventCreateWithFlags(&st.ev_obs, hipEventDisableTiming));
	while ((int)st.ev_comp.size() < nr) {
		hipEvent_t e;
		HIPCHK(obs, hipEventCreateWithFlags(&e, hipEventDisableTiming));
		st.ev_comp.push_back(e);
	}

	// start-up: lp of x0 in two half-batches through the same two entries, then the one host wait before the steps
	HIPCHK(obs, hipMemcpyAsync(st.x, x0, wd * sizeof(double), hipMemcpyHostToDevice, obs->stream));
	HIPCHK(obs, hipMemsetAsync(st.nacc, 0, (size_t)W * sizeof(int), obs->stream));
	for (int half = 0; half < 2; half++) {
		const double *xh = st.x + (size_t)half * h * d;
		if ((rc = sample_loglik(comp, nr, obs, h, xh))) return rc;
		if ((rc = gpemu_sample_logpost_dev(obs, h, d, xh, st.stat + h, st.lp + (size_t)half * h))) return rc;
	}
	HIPCHK(obs, hipMemcpyAsync(lp_end, st.lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, obs->stream));
	HIPCHK(obs, hipStreamSynchronize(obs->stream));
	for (int k = 0; k < W; k++)
		if (!std::isfinite(lp_end[k])) return fail(obs, GPEMU_ERR_ARG, "gpemu_calib_sample: a start has a non-finite log posterior");

	size_t filled = 0, done = 0;    // records staged in the chunk, records already copied out
	auto flush = [&]() -> int {
		if (trace_x) HIPCHK(obs, hipMemcpyAsync(trace_x + done * wd, st.trx, filled * wd * sizeof(double), hipMemcpyDeviceToHost, obs->stream));
		if (trace_lp) HIPCHK(obs, hipMemcpyAsync(trace_lp + done * W, st.trlp, filled * W * sizeof(double), hipMemcpyDeviceToHost, obs->stream));
		HIPCHK(obs, hipStreamSynchronize(obs->stream));
		done += filled;
		filled = 0;
		return GPEMU_OK;
	};
	for (int t = 0; t < args->nsteps; t++) {
		const unsigned long long g = g0 + (unsigned long long)t;
		for (int half = 0; half < 2; half++) {
			if ((rc = gpemu_sample_propose_dev(obs, W, d, half, g, args->seed, args->a, st.x, st.y, st.aux))) return rc;
			if ((rc = sample_loglik(comp, nr, obs, h, st.y))) return rc;
			if ((rc = gpemu_sample_accept_dev(obs, W, d, half, g, args->seed, st.y, st.aux, st.stat + h, st.x, st.lp, st.nacc))) return rc;
		}
		if (keep && recorded(g)) {
			HIPCHK(obs, hipMemcpyAsync(st.trx + filled * wd, st.x, wd * sizeof(double), hipMemcpyDeviceToDevice, obs->stream));
			HIPCHK(obs, hipMemcpyAsync(st.trlp + filled * W, st.lp, (size_t)W * sizeof(double), hipMemcpyDeviceToDevice, obs->stream));
			if (++filled == chunk && (rc = flush())) return rc;
		}
	}
	if (filled && (rc = flush())) return rc;
	HIPCHK(obs, hipMemcpyAsync(x_end, st.x, wd * sizeof(double), hipMemcpyDeviceToHost, obs->stream));
	HIPCHK(obs, hipMemcpyAsync(lp_end, st.lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, obs->stream));
	HIPCHK(obs, hipMemcpyAsync(naccept, st.nacc, (size_t)W * sizeof(int), hipMemcpyDeviceToHost, obs->stream));
	HIPCHK(obs, hipStreamSynchronize(obs->stream));
	*nrec_out = nrec;
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------
extern "C" int gpemu_prof_begin(gpemu_ctx *ctx, int cls)
{
	if (!ctx) return GPEMU_ERR_ARG;
	for (auto e : ctx->prof.ev) hipEventDestroy(e);
	ctx->prof.ev.clear();
	ctx->prof.cls = cls; ctx->prof.flops = ctx->prof.bytes = 0; ctx->prof.n = 0;
	ctx->prof.tag.clear();
	return GPEMU_OK;
}

extern "C" int gpemu_prof_end(gpemu_ctx *ctx, int *nlaunches, double *total_ms, double *flops, double *bytes)
{
	if (!ctx) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	double ms = 0.0;
	const bool dump = getenv("GPEMU_PROF_DUMP") != nullptr;
	for (size_t i = 0; i + 1 < ctx->prof.ev.size(); i += 2) {
		float t = 0.f;
		hipEventElapsedTime(&t, ctx->prof.ev[i], ctx->prof.ev[i + 1]);
		ms += t;
		if (dump && i / 2 < ctx->prof.tag.size()) fprintf(stderr, "[gpemu prof] %s ms=%.4f\n", ctx->prof.tag[i / 2].c_str(), t);
	}
	ctx->prof.tag.clear();
	if (nlaunches) *nlaunches = ctx->prof.n;
	if (total_ms) *total_ms = ms;
	if (flops) *flops = ctx->prof.flops;
	if (bytes) *bytes = ctx->prof.bytes;
	for (auto e : ctx->prof.ev) hipEventDestroy(e);
	ctx->prof.ev.clear();
	ctx->prof.cls = GPEMU_PROF_NONE;
	return GPEMU_OK;
}

// GPEMU_TRACE=1: write "tag start_ns end_ns" per kernel launch of the last factorisation (device wall clock,
// 100 MHz ticks converted to ns; the same clock for every context of a GPU) to a text file
extern "C" int gpemu_trace_dump(gpemu_ctx *ctx, const char *path)
{
	if (!ctx || !path) return GPEMU_ERR_ARG;
	if (!ctx->dTrace) { ctx->err = "tracing is off (set GPEMU_TRACE=1 before gpemu_ctx_create)"; return GPEMU_ERR_STATE; }
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<unsigned long long> h(8 * (size_t)ctx->trace_next);
	if (!h.empty()) {
		HIPCHK(ctx, hipMemcpyAsync(h.data(), ctx->dTrace, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	FILE *f = fopen(path, "w");
	if (!f) { ctx->err = "cannot open trace file"; return GPEMU_ERR_ARG; }
	for (int i = 0; i < ctx->trace_next; i++) {
		const unsigned long long *q = &h[8 * (size_t)i];
		if (q[3] == 0) continue;
		fprintf(f, "%s | %llu %llu %llu %llu %llu %llu %llu %llu\n", ctx->trace_tag[i].c_str(), ~q[0] * 10ull, q[1] * 10ull,
		        q[2] * 10ull, q[3], q[4], q[5], q[6], q[7]);
	}
	fclose(f);
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// low-level compatibility entries: the reference's libRbind-era interface passes N x N matrices through host
// memory (emulate-fns.c:275-299, regression.c:120-176, emulator.c:672-785).  The O(N^2)/O(N^3) work still runs here.
// ---------------------------------------------------------------------------
// The two matrix-only entries (gpemu_chol_inverse, gpemu_test_potrf) factor ONE n x n matrix of the caller's in buffers of their
// own, through a view over them, on the calling context's stream and with its switches; its model and workspace stay untouched.
// C -> C^-1 in place (both triangles), log det C = 2 sum log L_ii; *info = 1-based index of the first pivot <= 0
extern "C" int gpemu_chol_inverse(gpemu_ctx *ctx, int n, double *a, int lda, double *logdet, int *info)
{
	if (!ctx || n < 1 || !a || lda < n) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = round_up(n, LEAF), Rp = 64;
	const size_t rows = (size_t)2 * Np + Rp, dim = (size_t)Np + Rp;
	std::vector<double> h((size_t)Np * Np, 0.0), diag((size_t)n);
	for (int i = 0; i < Np; i++)
		for (int j = 0; j <= i; j++)
			h[(size_t)i * Np + j] = (i < n) ? a[(size_t)i * lda + j] : (i == j ? 1.0 : 0.0);
	int big = INFO_NONE, inf = 0;
	DevBuf<double> dT, dS;
	DevBuf<int> dInfo;
	HIPCHK(ctx, dT.grow(rows * Np));
	HIPCHK(ctx, dInfo.grow(1));
	HIPCHK(ctx, dS.grow(dim * dim));
	const Tall t{dT, dInfo, Np, Rp, 1, (long)(rows * Np)};
	HIPCHK(ctx, trace_clear(ctx));
	HIPCHK(ctx, hipMemcpyAsync(dT, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemsetAsync(dT + (size_t)Np * Np, 0, (size_t)Rp * Np * 8, ctx->stream));
	HIPCHK(ctx, launch_set_identity_rows(ctx->stream, dT + (size_t)(Np + Rp) * Np, Np, Np));
	HIPCHK(ctx, hipMemcpyAsync(dInfo, &big, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, potrf_all(ctx, t, 1));
	HIPCHK(ctx, hipMemcpyAsync(&inf, dInfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(diag.data(), sizeof(double), dT, ((size_t)Np + 1) * sizeof(double), sizeof(double), n,
	                             hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	const int bad = pivot_info(inf);
	if (!bad) {
		HIPCHK(ctx, build_corner(ctx, t, dS, (long)dim));   // C^-1 = U U^T, lower triangle at (Rp, Rp) of the corner
		HIPCHK(ctx, hipMemcpy2DAsync(a, (size_t)lda * sizeof(double), dS + (size_t)Rp * dim + Rp, dim * sizeof(double),
		                             (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	if (info) *info = bad;
	if (bad) return fail(ctx, GPEMU_ERR_NOT_PD, "matrix is not positive definite");
	double ld = 0.0;
	for (int i = 0; i < n; i++) ld += log(diag[i]);
	if (logdet) *logdet = 2.0 * ld;
	for (int i = 0; i < n; i++)
		for (int j = i + 1; j < n; j++) a[(size_t)i * lda + j] = a[(size_t)j * lda + i];
	return GPEMU_OK;
}

// 64-bit checksum of every element of a host matrix (four independent multiply-xor lanes, one pass at memory speed):
// decides whether the device copy of a caller's C^-1 is still current.  The callers (libRbind-style loops,
// libEmu/regression.c:120-176 and emulator.c:672-785 callers) reuse ONE cinverse buffer and rewrite it in place, so
// pointer and sizes alone say nothing; a sampled fingerprint could miss an interior change.
static uint64_t matrix_checksum(const double *a, int n, int lda)
{
	uint64_t h[4] = {0x9E3779B97F4A7C15ull, 0xBF58476D1CE4E5B9ull, 0x94D049BB133111EBull, 0xD6E8FEB86659FD93ull};
	const uint64_t K = 0xFF51AFD7ED558CCDull;
	for (int i = 0; i < n; i++) {
		const double *row = a + (size_t)i * lda;
		int j = 0;
		for (; j + 4 <= n; j += 4) {
			uint64_t w[4];
			memcpy(w, row + j, sizeof w);
			h[0] = (h[0] ^ w[0]) * K; h[1] = (h[1] ^ w[1]) * K; h[2] = (h[2] ^ w[2]) * K; h[3] = (h[3] ^ w[3]) * K;
		}
		for (; j < n; j++) {
			uint64_t w;
			memcpy(&w, row + j, sizeof w);
			h[j & 3] = (h[j & 3] ^ w) * K;
		}
		h[0] ^= h[0] >> 29;                                 // row boundary: position-dependent
	}
	uint64_t r = h[0];
	for (int k = 1; k < 4; k++) r = (r ^ (h[k] + (r << 6) + (r >> 2))) * K;
	return r ^ (r >> 32);
}

// forget the cached device copy of the host matrix: the next gpemu_symm_apply uploads without comparing checksums
// (not needed for correctness; saves a caller that knows it has rewritten the buffer one pass over it)
extern "C" int gpemu_symm_invalidate(gpemu_ctx *ctx)
{
	if (!ctx) return GPEMU_ERR_ARG;
	ctx->sym_key = nullptr;
	ctx->sym_pinned = false;
	return GPEMU_OK;
}

// pinned = 1: the caller promises not to modify the matrix it passes to gpemu_symm_apply / gpemu_trace_product until it
// unpins (or invalidates): calls with the same (pointer, n, lda) then skip the per-call checksum pass (one read of
// N x N doubles from host memory -- 0.1 s at N = 8192, far more than the device product it guards).  The reference's
// per-point loops (makeEmulatedMean / makeEmulatedVariance over one cinverse, emulator.c:672-785) are such callers.
extern "C" int gpemu_symm_pin(gpemu_ctx *ctx, int pinned)
{
	if (!ctx) return GPEMU_ERR_ARG;
	ctx->sym_pinned = pinned != 0;
	return GPEMU_OK;
}

// out[v][i] = sum_j A[i][j] V[v][j] for nvec vectors stored as rows; A symmetric, host-resident, N x N with row
// stride lda.  A is uploaded when (pointer, sizes) differ from the cached copy, or -- unless pinned -- when the checksum
// of all its elements does (the checksum pass runs only when pointer and sizes match: a new matrix is uploaded at once).
extern "C" int gpemu_symm_apply(gpemu_ctx *ctx, int n, const double *a, int lda, int nvec, const double *v, double *out)
{
	if (!ctx || n < 1 || !a || lda < n || nvec < 1 || !v || !out) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Npad = round_up(n, 64);
	const bool same_key = ctx->dSym && ctx->sym_key == a && ctx->sym_N == n && ctx->sym_lda == lda;
	bool current = same_key && ctx->sym_pinned;
	uint64_t fp = 0;
	if (same_key && !current) {
		fp = matrix_checksum(a, n, lda);
		current = fp == ctx->sym_fp;
	}
	if (!current) {
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		const int rc = grow(ctx, ctx->dSym, (size_t)Npad * Npad);
		if (rc) return rc;
		ctx->sym_pad = Npad;
		HIPCHK(ctx, hipMemsetAsync(ctx->dSym, 0, (size_t)Npad * Npad * sizeof(double), ctx->stream));
		HIPCHK(ctx, hipMemcpy2DAsync(ctx->dSym, (size_t)Npad * sizeof(double), a, (size_t)lda * sizeof(double),
		                             (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, ctx->stream));
		if (!same_key) fp = matrix_checksum(a, n, lda);      // (a new matrix: its checksum for the calls that follow)
		ctx->sym_key = a; ctx->sym_N = n; ctx->sym_lda = lda; ctx->sym_fp = fp;
	}
	const size_t vlen = (size_t)round_up(nvec, 64) * Npad;
	int rc = grow(ctx, ctx->dSymV, vlen);
	if (!rc) rc = grow(ctx, ctx->dSymOut, vlen);
	if (rc) return rc;
	HIPCHK(ctx, hipMemsetAsync(ctx->dSymV, 0, (size_t)nvec * Npad * sizeof(double), ctx->stream));
	HIPCHK(ctx, hipMemcpy2DAsync(ctx->dSymV, (size_t)Npad * sizeof(double), v, (size_t)n * sizeof(double),
	                             (size_t)n * sizeof(double), nvec, hipMemcpyHostToDevice, ctx->stream));
	GemmArgs g{};
	g.C = ctx->dSymOut; g.ldc = Npad;
	g.A = ctx->dSymV; g.lda = Npad;
	g.B = ctx->dSym; g.ldb = Npad;
	g.m = nvec; g.n = Npad; g.k0 = 0; g.k1 = Npad; g.alpha = 1.0; g.beta = 0;
	HIPCHK(ctx, gemm(ctx, g));
	HIPCHK(ctx, hipMemcpy2DAsync(out, (size_t)n * sizeof(double), ctx->dSymOut, (size_t)Npad * sizeof(double),
	                             (size_t)n * sizeof(double), nvec, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// a5 derivative_l_gauss (libEmu/emulator.c:173-209) materialised into host memory: the N x N matrix of the literal
// one-coordinate formula for the design column xcol[n] and the log length scale theta_len
extern "C" int gpemu_derivative_gauss(gpemu_ctx *ctx, int n, const double *xcol, double theta_len, double *out, int ldo)
{
	if (!ctx || n < 1 || !xcol || !out || ldo < n) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dx, dout;
	HIPCHK(ctx, dx.grow((size_t)n));
	HIPCHK(ctx, dout.grow((size_t)n * n));
	HIPCHK(ctx, hipMemcpyAsync(dx, xcol, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, launch_deriv_gauss(ctx->stream, dout, n, dx, n, theta_len));
	HIPCHK(ctx, hipMemcpy2DAsync(out, (size_t)ldo * sizeof(double), dout, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n,
	                             hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// trace(A B) = sum_ij A[i][j] B[j][i] of two host-resident n x n matrices (row strides lda, ldb): getGradientCn's
// trace(C^-1 dC/dtheta) (libEmu/maxmultimin.c:583-588) as one pass over the two matrices instead of an N^3 dgemm.
// A goes through the same cache as gpemu_symm_apply -- literally: the gpemu_symm_apply call below is what makes it
// resident, with that entry's (pointer, size, checksum, pin) rules; B is uploaded on every call.
extern "C" int gpemu_trace_product(gpemu_ctx *ctx, int n, const double *a, int lda, const double *b, int ldb, double *trace)
{
	if (!ctx || n < 1 || !a || !b || lda < n || ldb < n || !trace) return GPEMU_ERR_ARG;
	std::vector<double> one((size_t)n, 0.0), tmp((size_t)n);
	int rc = gpemu_symm_apply(ctx, n, a, lda, 1, one.data(), tmp.data());      // makes sure a is resident in dSym
	if (rc) return rc;
	const int Npad = ctx->sym_pad;
	DevBuf<double> dB, dPart;
	HIPCHK(ctx, dB.grow((size_t)Npad * Npad));
	HIPCHK(ctx, dPart.grow((size_t)n));
	HIPCHK(ctx, hipMemcpy2DAsync(dB, (size_t)Npad * sizeof(double), b, (size_t)ldb * sizeof(double), (size_t)n * sizeof(double), n,
	                             hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, launch_trace_product(ctx->stream, ctx->dSym, dB, Npad, n, dPart));
	HIPCHK(ctx, hipMemcpyAsync(tmp.data(), dPart, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	double t = 0.0;
	for (int i = 0; i < n; i++) t += tmp[i];
	*trace = t;
	return GPEMU_OK;
}

// ---------------------------------------------------------------------------
// building blocks exported for the parity tests
// ---------------------------------------------------------------------------
extern "C" int gpemu_test_gemm_nt(gpemu_ctx *ctx, int m, int n, int k, double alpha, int beta, const double *a,
                                  const double *b, double *c)
{
	if (!ctx || m < 1 || n < 1 || k < 1 || (k % GEMM_BK) != 0) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> da, db, dc;
	HIPCHK(ctx, da.grow((size_t)m * k));
	HIPCHK(ctx, db.grow((size_t)n * k));
	HIPCHK(ctx, dc.grow((size_t)m * n));
	HIPCHK(ctx, hipMemcpyAsync(da, a, (size_t)m * k * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(db, b, (size_t)n * k * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dc, c, (size_t)m * n * 8, hipMemcpyHostToDevice, ctx->stream));
	GemmArgs g{};
	g.C = dc; g.A = da; g.B = db; g.ldc = n; g.lda = k; g.ldb = k; g.m = m; g.n = n; g.k0 = 0; g.k1 = k;
	g.alpha = alpha; g.beta = beta;
	HIPCHK(ctx, gemm(ctx, g));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(c, dc, (size_t)m * n * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// One gemm() call with caller-chosen GemmArgs on operands that live in ONE host buffer, the arena (C, A and B at element
// offsets, as in production, where C sits in the same tall workspace as A and B): uploads the whole arena, applies the
// context's Sched exactly as gemm() does (force_cfg on top), launches, and downloads the whole arena, so that a test sees
// every element the launch must and must not have touched.
// What the kernel may address is computed here first, and anything outside [0, arena_len) is refused: operand rows are
// clamped to m-1 / n-1, only the columns [k0, k1) of A and B are read, and rows < m, columns < n of each of the
// max(nbatch, ksplit, 1) C blocks are read (beta) and written.  Everything launch_gemm refuses, and what it takes on
// trust (k0, k1 multiples of 16, k1 > k0), comes back as GPEMU_ERR_ARG as well.
// The skipping modes drop k-blocks on the ASSUMPTION that the operand is zero there; the caller owes the kernel
//   kstart_mode: A[i][k] = 0 for k < i - kstart_off   (the rows of [Z^T; U], build_corner: kstart_off dense rows first)
//   kend_mode:   B[j][k] = 0 for k > j - kend_off     (the rows of L^-1; rows j >= k1 behind them are dense)
// and the result equals the full product over [k0, k1) only under them.
// fa: one info word per matrix, INFO_NONE before the launch, decoded by pivot_info afterwards (as gpemu_test_potrf); a
// launch that would not take the factor-ahead tile is refused, never run without it.
extern "C" int gpemu_test_gemm_launch(gpemu_ctx *ctx, double *arena, long arena_len, const gpemu_gemm_launch_args *p, int *info_out)
{
	if (!ctx || !arena || !p) return GPEMU_ERR_ARG;
	constexpr long DIM_MAX = 1L << 20, LD_MAX = 1L << 24, LEN_MAX = 1L << 32, STRIDE_MAX = 1L << 32;   // no product below leaves 63 bits
	if (arena_len < 1 || arena_len > LEN_MAX) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: arena length");
	if (p->m < 1 || p->n < 1 || p->m > DIM_MAX || p->n > DIM_MAX) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: m, n");
	if (p->k0 < 0 || p->k1 <= p->k0 || p->k1 > DIM_MAX || (p->k0 % GEMM_BK) != 0 || (p->k1 % GEMM_BK) != 0)
		return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: k0, k1 must be multiples of 16 with k0 < k1");
	if (p->beta != 0 && p->beta != 1) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: beta is 0 or 1");
	if (p->beta && p->alpha != 1.0 && p->alpha != -1.0) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: beta = 1 needs alpha = +-1");
	if (p->force_cfg != 0 && p->force_cfg != 2 && p->force_cfg != 8) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: force_cfg is 0, 2 or 8");
	if (p->nbatch < 0 || p->nbatch > GPEMU_MAX_BATCH || p->ksplit < 0 || p->ksplit > GPEMU_MAX_BATCH)
		return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: nbatch, ksplit");
	if (p->ksplit > 1 && (p->beta || p->nbatch > 1)) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: split-K takes beta = 0 and one problem");
	if ((p->tri != 0 && p->tri != 1) || (p->kstart_mode != 0 && p->kstart_mode != 1) || (p->kend_mode != 0 && p->kend_mode != 1) ||
	    (p->fa != 0 && p->fa != 1) || p->kstart_off < 0 || p->kstart_off > DIM_MAX || p->kend_off < 0 || p->kend_off > DIM_MAX ||
	    p->fa_c0 < 0 || p->fa_c0 > DIM_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: mode flags");
	if (p->ldc < 1 || p->lda < 1 || p->ldb < 1 || p->ldc > LD_MAX || p->lda > LD_MAX || p->ldb > LD_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: leading dimensions");
	if (std::labs(p->bsC) > STRIDE_MAX || std::labs(p->bsA) > STRIDE_MAX || std::labs(p->bsB) > STRIDE_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: batch strides");
	const bool split = p->ksplit > 1;
	const int nblk = std::max(std::max(p->nbatch, p->ksplit), 1);
	// smallest and largest element index of one operand over all blocks (the stride may have either sign)
	auto inside = [&](long off, long stride, long first, long last) {
		const long s0 = 0, s1 = (long)(nblk - 1) * stride;
		return off >= 0 && off <= arena_len && off + first + std::min(s0, s1) >= 0 && off + last + std::max(s0, s1) < arena_len;
	};
	if (!inside(p->offC, p->bsC, 0, (long)(p->m - 1) * p->ldc + p->n - 1) ||
	    !inside(p->offA, split ? 0 : p->bsA, p->k0, (long)(p->m - 1) * p->lda + p->k1 - 1) ||
	    !inside(p->offB, split ? 0 : p->bsB, p->k0, (long)(p->n - 1) * p->ldb + p->k1 - 1))
		return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: the launch would address memory outside the arena");

	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dArena;
	DevBuf<int> dInfo;
	HIPCHK(ctx, dArena.grow((size_t)arena_len));
	HIPCHK(ctx, dInfo.grow((size_t)nblk));
	GemmArgs g{};
	g.C = dArena + p->offC; g.A = dArena + p->offA; g.B = dArena + p->offB;
	g.ldc = p->ldc; g.lda = p->lda; g.ldb = p->ldb; g.m = p->m; g.n = p->n; g.k0 = p->k0; g.k1 = p->k1;
	g.alpha = p->alpha; g.beta = p->beta; g.tri = p->tri;
	g.kstart_mode = p->kstart_mode; g.kstart_off = p->kstart_off; g.kend_mode = p->kend_mode; g.kend_off = p->kend_off;
	g.bsC = p->bsC; g.bsA = p->bsA; g.bsB = p->bsB; g.nbatch = p->nbatch; g.ksplit = p->ksplit;
	g.force_cfg = p->force_cfg; g.fa = p->fa; g.fa_c0 = p->fa_c0; g.fa_info = dInfo;
	if (g.fa) {
		GemmArgs probe = g;
		apply_sched(ctx->sched, probe);
		if (!gemm_factor_ahead_ok(probe)) return fail(ctx, GPEMU_ERR_ARG, "gemm_launch: this launch would not take the factor-ahead tile");
	}
	std::vector<int> inf((size_t)nblk, INFO_NONE);
	HIPCHK(ctx, hipMemcpyAsync(dArena, arena, (size_t)arena_len * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dInfo, inf.data(), (size_t)nblk * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, gemm(ctx, g));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(arena, dArena, (size_t)arena_len * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(inf.data(), dInfo, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if (info_out)
		for (int b = 0; b < std::max(p->nbatch, 1); b++) info_out[b] = pivot_info(inf[(size_t)b]);
	return GPEMU_OK;
}

// One trailing_update() call -- the routine every factorisation calls, unchanged, with its split into matrix rows,
// right-hand-side rows (a launch of their own, or riders in the first) and identity rows -- on tall matrices inside ONE host
// buffer, the arena: uploads the whole arena, runs the update with the context's Sched (`ride` passed to trailing_update in place of GPEMU_RHS_RIDE
// for this call), downloads the whole arena.  The tall matrix is what Tall describes: ld matrix rows of ld columns, rp
// right-hand-side rows under them, and with inv the identity rows under those, of which the update takes c0+k.
// Footprint per matrix, checked against [0, arena_len) first: rows c0+k .. ld+rp(+c0+k)-1 of columns c0 .. c0+k+ncols-1.
// The kernels move 16-byte pieces of rows: off, ld, stride and c0 must be even, k a multiple of 16.
extern "C" int gpemu_test_update_launch(gpemu_ctx *ctx, double *arena, long arena_len, const gpemu_update_launch_args *p, int *info_out)
{
	if (!ctx || !arena || !p) return GPEMU_ERR_ARG;
	constexpr long DIM_MAX = 1L << 20, LEN_MAX = 1L << 32, STRIDE_MAX = 1L << 32;   // no product below leaves 63 bits
	if (arena_len < 1 || arena_len > LEN_MAX) return fail(ctx, GPEMU_ERR_ARG, "update_launch: arena length");
	if (p->ld < 1 || p->ld > DIM_MAX || p->rp < 0 || p->rp > DIM_MAX || (p->inv != 0 && p->inv != 1) || (p->ride != 0 && p->ride != 1))
		return fail(ctx, GPEMU_ERR_ARG, "update_launch: ld, rp, inv, ride");
	if (p->c0 < 0 || p->k < GEMM_BK || (p->k % GEMM_BK) != 0 || p->ncols < 1 || (long)p->c0 + p->k + p->ncols > p->ld)
		return fail(ctx, GPEMU_ERR_ARG, "update_launch: c0 >= 0, k a multiple of 16, ncols >= 1, c0 + k + ncols <= ld");
	if (p->rhs_live < 0 || p->rhs_live > p->rp) return fail(ctx, GPEMU_ERR_ARG, "update_launch: rhs_live is 0 .. rp");
	if (p->nbatch < 0 || p->nbatch > GPEMU_MAX_BATCH || p->stride < 0 || p->stride > STRIDE_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "update_launch: nbatch, stride");
	if (p->off < 0 || ((p->off | p->ld | p->stride | p->c0) & 1)) return fail(ctx, GPEMU_ERR_ARG, "update_launch: off, ld, stride and c0 must be even");
	const int nb = std::max(p->nbatch, 1);
	const long r0 = (long)p->c0 + p->k, row_end = p->ld + p->rp + (p->inv ? r0 : 0);
	const long last = p->off + (long)(nb - 1) * p->stride + (row_end - 1) * p->ld + r0 + p->ncols - 1;
	if (last >= arena_len) return fail(ctx, GPEMU_ERR_ARG, "update_launch: the update would address memory outside the arena");
	if (nb > 1 && p->stride < (row_end - 1) * p->ld + r0 + p->ncols)
		return fail(ctx, GPEMU_ERR_ARG, "update_launch: the matrices of the batch overlap");

	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dArena;
	DevBuf<int> dInfo;
	HIPCHK(ctx, dArena.grow((size_t)arena_len));
	HIPCHK(ctx, dInfo.grow((size_t)nb));
	std::vector<int> inf((size_t)nb, INFO_NONE);
	HIPCHK(ctx, hipMemcpyAsync(dArena, arena, (size_t)arena_len * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dInfo, inf.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	const Tall t{dArena + p->off, dInfo, (int)p->ld, p->rp, nb, (long)p->stride, p->rhs_live};
	bool fa_done = false;
	HIPCHK(ctx, trailing_update(ctx, t, p->c0, p->k, p->ncols, p->inv, &fa_done, 0, p->ride));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(arena, dArena, (size_t)arena_len * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(inf.data(), dInfo, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if (info_out)
		for (int b = 0; b < nb; b++) info_out[b] = pivot_info(inf[(size_t)b]);
	return GPEMU_OK;
}

// One launch_leaf / launch_leaf_pair call -- the launchers production calls, unchanged -- with caller-chosen arguments on a
// matrix (or a lock-step batch of them, bstride elements apart) inside ONE host buffer, the arena: uploads the whole arena,
// launches, downloads the whole arena, so that a test sees every element the launch must and must not have touched.
//   GPEMU_LEAF_FACTOR        leaf_factor_kernel on the 64x64 block at (c0, c0)                       (m_below = 0)
//   GPEMU_LEAF_SOLVE         leaf_solve_kernel<staged, pre> on the m_below rows under a FACTORED block (skip_factor)
//   GPEMU_LEAF_FACTOR_SOLVE  both, the plain leaf
//   GPEMU_LEAF_PAIR          leaf_pair_kernel: solve of columns [c0, c0+64) and K = 64 update of [c0+64, c0+128), fa: with
//                            the factor-ahead tile
//   GPEMU_LEAF_PANEL_ROWS    panel_rows_kernel (launch_panel_rows): the m_far rows from r_far on under the finished 256-column
//                            group at c0; footprint per matrix: the square, rows and columns c0 .. c0+255, and rows
//                            r_far .. r_far+m_far-1 of those columns
// What the kernels may address is computed here first and anything outside [0, arena_len) is refused: per matrix rows
// c0 .. c0+64+m_below-1 of columns c0 .. c0+63 (the pair: .. c0+127; the row clamps of the solve stay inside m_below), and
// with c0b >= 0 rows c0b .. c0b+127 of columns c0b .. c0b+63.  The staged solve and the pair move 16-byte pieces of rows:
// off, ld, bstride, c0 and c0b must be even (production: Np and the strides are multiples of 64).
// Info: one word per matrix, INFO_NONE before the launch, decoded by pivot_info afterwards.
extern "C" int gpemu_test_leaf_launch(gpemu_ctx *ctx, double *arena, long arena_len, const gpemu_leaf_launch_args *p, int *info_out)
{
	if (!ctx || !arena || !p || !info_out) return GPEMU_ERR_ARG;
	constexpr long DIM_MAX = 1L << 20, LD_MAX = 1L << 24, LEN_MAX = 1L << 32, STRIDE_MAX = 1L << 32;   // no product below leaves 63 bits
	if (arena_len < 1 || arena_len > LEN_MAX) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: arena length");
	if (p->op != GPEMU_LEAF_FACTOR && p->op != GPEMU_LEAF_SOLVE && p->op != GPEMU_LEAF_FACTOR_SOLVE && p->op != GPEMU_LEAF_PAIR &&
	    p->op != GPEMU_LEAF_PANEL_ROWS)
		return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: op");
	const bool far = p->op == GPEMU_LEAF_PANEL_ROWS;
	if (!far && (p->r_far != 0 || p->m_far != 0)) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: r_far and m_far belong to the panel rows");
	if (far && (p->m_below != 0 || p->c0b >= 0 || p->fa)) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the panel rows take m_below = 0, no c0b, no fa");
	if (far && (p->m_far < LEAF || p->m_far > DIM_MAX || p->m_far % LEAF)) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the panel rows take m_far = 64, 128, ...");
	if (far && (p->r_far > DIM_MAX || p->r_far < p->c0 + 4 * LEAF)) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the panel rows start at r_far >= c0 + 256");
	if (p->staged < -1 || p->staged > 1 || (p->pre != 0 && p->pre != 1) || (p->fa != 0 && p->fa != 1) || p->c0b < -1 || p->c0b > DIM_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: staged is -1/0/1, pre and fa are 0/1, c0b is -1 or a column");
	if (p->nbatch < 0 || p->nbatch > GPEMU_MAX_BATCH) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: nbatch");
	if (p->off < 0 || p->off > arena_len || p->ld < 1 || p->ld > LD_MAX || p->c0 < 0 || p->c0 > DIM_MAX || p->m_below < 0 ||
	    p->m_below > DIM_MAX || std::labs(p->bstride) > STRIDE_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: off, ld, c0, m_below, bstride");
	const bool pair = p->op == GPEMU_LEAF_PAIR, solves = p->op == GPEMU_LEAF_SOLVE || p->op == GPEMU_LEAF_FACTOR_SOLVE;
	if (p->op == GPEMU_LEAF_FACTOR && p->m_below != 0) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the factor alone takes m_below = 0");
	if (pair && (p->m_below < LEAF || p->m_below % LEAF)) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the pair takes m_below = 64, 128, ...");
	if (solves && p->m_below < 1) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: a solve needs m_below >= 1");
	if ((p->off & 1) || (p->ld & 1) || (p->bstride & 1) || (p->c0 & 1) || (p->c0b >= 0 && (p->c0b & 1)))
		return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: off, ld, bstride, c0 and c0b must be even (16-byte row pieces)");
	if (p->c0b >= 0 && !solves) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: c0b needs an op that launches the solve");
	if (p->fa && !pair) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: fa belongs to the pair");
	const int width = far ? 4 * LEAF : pair ? 2 * LEAF : LEAF;
	if (p->c0 + width > p->ld || (p->c0b >= 0 && p->c0b + LEAF > p->ld)) return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the columns leave the row");
	const int nblk = std::max(p->nbatch, 1);
	// smallest and largest element index over all matrices (the stride may have either sign)
	auto inside = [&](long first, long last) {
		const long s0 = 0, s1 = (long)(nblk - 1) * p->bstride;
		return p->off + first + std::min(s0, s1) >= 0 && p->off + last + std::max(s0, s1) < arena_len;
	};
	const long last_row = far ? (long)p->r_far + p->m_far - 1 : (long)p->c0 + LEAF + p->m_below - 1;
	if (!inside((long)p->c0 * p->ld + p->c0, last_row * p->ld + p->c0 + width - 1) ||
	    (p->c0b >= 0 && !inside((long)p->c0b * p->ld + p->c0b, (long)(p->c0b + 2 * LEAF - 1) * p->ld + p->c0b + LEAF - 1)))
		return fail(ctx, GPEMU_ERR_ARG, "leaf_launch: the launch would address memory outside the arena");

	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dArena;
	DevBuf<int> dInfo;
	HIPCHK(ctx, dArena.grow((size_t)arena_len));
	HIPCHK(ctx, dInfo.grow((size_t)nblk));
	std::vector<int> inf((size_t)nblk, INFO_NONE);
	HIPCHK(ctx, hipMemcpyAsync(dArena, arena, (size_t)arena_len * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dInfo, inf.data(), (size_t)nblk * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	double *T = dArena + p->off;
	if (far) HIPCHK(ctx, launch_panel_rows(ctx->stream, T, p->ld, p->c0, p->r_far, p->m_far, nullptr, p->nbatch, p->bstride));
	else if (pair) HIPCHK(ctx, launch_leaf_pair(ctx->stream, T, p->ld, p->c0, p->m_below, dInfo, nullptr, p->nbatch, p->bstride, p->fa != 0));
	else HIPCHK(ctx, launch_leaf(ctx->stream, T, p->ld, p->c0, p->m_below, dInfo, nullptr, nullptr, p->nbatch, p->bstride,
	                             p->op == GPEMU_LEAF_SOLVE, p->staged, p->pre != 0, p->c0b));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(arena, dArena, (size_t)arena_len * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(inf.data(), dInfo, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	for (int b = 0; b < nblk; b++) info_out[b] = pivot_info(inf[(size_t)b]);
	return GPEMU_OK;
}

// The gradient reductions behind the corners (grad_sums_of_corners: the routine grad_enqueue_chunk calls) ONCE, on corners,
// [y|H] columns and Gram matrices the caller chose, for the model and mode the context holds.  The corners are laid out on
// the host as production's S is -- side Np + Rp, S[Rp+i][Rp+j] = a[i][j] for j <= i, S[Rp+i][0 .. nreg] = z[i] -- and every
// other element of them is NaN, as are the alpha slots beyond N, the beta slots beyond nreg, the Gram matrices outside
// their (1 + nreg)^2 corner, the tile sums and the second-stage sums before the launch: what the kernels must not read
// shows in the outputs, what they do not write stays NaN.  All device buffers are the call's own; of the context it
// reads the design (dX, dXg), the model's sizes, the mode and the schedule switch, and uses the stream.
extern "C" int gpemu_test_grad_sums(gpemu_ctx *ctx, const gpemu_grad_sums_args *p)
{
	if (!ctx || !p) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	if (p->nb < 1 || p->nb > GPEMU_MAX_BATCH) return fail(ctx, GPEMU_ERR_ARG, "grad_sums: batch size must be 1..GPEMU_MAX_BATCH");
	if ((p->form != 0 && p->form != 1) || p->gram_dist < -1 || p->gram_dist > 1 || p->clamp < -1 || p->clamp > 1)
		return fail(ctx, GPEMU_ERR_ARG, "grad_sums: form is 0/1, gram_dist and clamp are -1/0/1");
	const bool exact = p->form == 1;
	if (!p->thetas || !p->a || !p->z || !p->alpha_out || !p->part_out || !p->sums_out || (exact && (!p->gram || !p->beta_out)))
		return fail(ctx, GPEMU_ERR_ARG, "grad_sums: NULL pointer");
	if (ctx->kind != GPEMU_POWEREXP) {
		if (!(ctx->mode & GPEMU_MODE_EXACT_GRAD) || !(ctx->mode & GPEMU_MODE_MATERN_LOG))
			return fail(ctx, GPEMU_ERR_ARG, "grad_sums: a Matern model needs GPEMU_MODE_EXACT_GRAD | GPEMU_MODE_MATERN_LOG");
		if (!exact) return fail(ctx, GPEMU_ERR_ARG, "grad_sums: there is no literal Matern gradient");
	}
	const int nb = p->nb, nthetas = p->nthetas;
	if (nthetas < nthetas_for(ctx) || nthetas > GPEMU_MAX_PARAMS + 2) return fail(ctx, GPEMU_ERR_ARG, "grad_sums: nthetas");
	const bool gram = exact && (p->gram_dist < 0 ? ctx->sched.grad_gram != 0 : p->gram_dist == 1);
	if (exact && p->gram_dist == 1 && !ctx->dXg) return fail(ctx, GPEMU_ERR_ARG, "grad_sums: no centred design for the Gram form");
	if (!exact && p->clamp == 0 && !grad_lit_noclamp(ctx, nb, p->thetas, nthetas))
		return fail(ctx, GPEMU_ERR_ARG, "grad_sums: the unclamped literal kernel is defined only where production's rule selects it");
	std::vector<CovParams> ps;
	int rc = make_cov_params_batch(ctx, nb, p->thetas, nthetas, &ps);
	if (rc) return rc;

	const int N = ctx->N, d = ctx->d, Np = ctx->Np, Rp = ctx->Rp, nreg = ctx->nreg, nz = 1 + nreg;
	const size_t dim = (size_t)Np + Rp, sstride = dim * dim;
	const size_t gslot = (size_t)Np + 2 * GPEMU_MAX_PARAMS;
	const int nt = (N + 63) / 64, ntiles = nt * (nt + 1) / 2, np = 2 * d + 2;
	const size_t need = (size_t)ntiles * np, rlen = (size_t)Rp * Rp;
	std::vector<double> hS((size_t)nb * sstride, NAN), hAg((size_t)nb * gslot, NAN), hPart(need * nb, NAN), hSums((size_t)nb * np, NAN);
	std::vector<double> hRes(exact ? (size_t)nb * rlen : 0, NAN), gph((size_t)nb * GPEMU_MAX_PARAMS, 0.0);
	for (int b = 0; b < nb; b++) {
		double *S = hS.data() + (size_t)b * sstride;
		const double *a = p->a + (size_t)b * N * N, *z = p->z + (size_t)b * N * nz;
		for (int i = 0; i < N; i++) {
			for (int j = 0; j <= i; j++) S[(size_t)(Rp + i) * dim + Rp + j] = a[(size_t)i * N + j];
			for (int c = 0; c < nz; c++) S[(size_t)(Rp + i) * dim + c] = z[(size_t)i * nz + c];
		}
		if (exact)
			for (int i = 0; i < nz; i++)
				for (int j = 0; j < nz; j++) hRes[(size_t)b * rlen + (size_t)i * Rp + j] = p->gram[((size_t)b * nz + i) * nz + j];
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dS, dAg, dPart, dSums, dRes;
	DevBuf<CovParams> dPp;
	HIPCHK(ctx, dS.grow(hS.size()));
	HIPCHK(ctx, dAg.grow(hAg.size()));
	HIPCHK(ctx, dPart.grow(hPart.size()));
	HIPCHK(ctx, dSums.grow(hSums.size()));
	HIPCHK(ctx, dRes.grow(std::max(hRes.size(), (size_t)1)));
	HIPCHK(ctx, dPp.grow((size_t)nb));
	HIPCHK(ctx, hipMemcpyAsync(dS, hS.data(), hS.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dAg, hAg.data(), hAg.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dPart, hPart.data(), hPart.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dSums, hSums.data(), hSums.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	if (exact) HIPCHK(ctx, hipMemcpyAsync(dRes, hRes.data(), hRes.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dPp, ps.data(), (size_t)nb * sizeof(CovParams), hipMemcpyHostToDevice, ctx->stream));
	GradWork w{};
	w.S = dS; w.ag = dAg; w.part = dPart; w.sums = dSums; w.sums_stride = np;
	w.res = dRes; w.rstride = (long)rlen; w.pp = dPp; w.gph = gph.data(); w.gph_ev = nullptr;
	w.exact = exact; w.gram = gram; w.clamp = p->clamp;
	rc = grad_sums_of_corners(ctx, w, nb, p->thetas, nthetas);
	// (the copies above and inside the routine read host vectors of this frame: wait before any return)
	const hipError_t es = hipStreamSynchronize(ctx->stream);
	if (rc) return rc;
	HIPCHK(ctx, es);
	HIPCHK(ctx, hipMemcpyAsync(hAg.data(), dAg, hAg.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(hPart.data(), dPart, hPart.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(hSums.data(), dSums, hSums.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	for (int b = 0; b < nb; b++) {
		memcpy(p->alpha_out + (size_t)b * N, hAg.data() + (size_t)b * gslot, (size_t)N * 8);
		if (exact) memcpy(p->beta_out + (size_t)b * nreg, hAg.data() + (size_t)b * gslot + Np + GPEMU_MAX_PARAMS, (size_t)nreg * 8);
	}
	memcpy(p->part_out, hPart.data(), hPart.size() * 8);
	memcpy(p->sums_out, hSums.data(), hSums.size() * 8);
	return GPEMU_OK;
}

// The matrix a lock-step batch is factored from: stages nb matrices exactly as gpemu_loglik_batch does (ONE launch of
// cov_stage_batch_kernel: lower tiles only, every matrix its own hyper-parameters) and copies the N x N block of matrix b
// to the host without factorising.  Tiles strictly above the diagonal are not written by that path (out keeps what the
// workspace held there).
extern "C" int gpemu_test_staged_matrix(gpemu_ctx *ctx, int nb, const double *thetas, int nthetas, int b, double *out)
{
	if (!ctx || !thetas || !out || nb < 1 || nb > GPEMU_MAX_BATCH || b < 0 || b >= nb) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	std::vector<CovParams> ps;
	int rc = make_cov_params_batch(ctx, nb, thetas, nthetas, &ps);
	if (rc) return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	invalidate_prediction(ctx);
	rc = stage_matrices(ctx, ps.data(), nb, 0);
	if (rc) return rc;
	const int N = ctx->N, Np = ctx->Np;
	HIPCHK(ctx, hipMemcpy2DAsync(out, (size_t)N * sizeof(double), ctx->dT + (size_t)b * ctx->T_stride, (size_t)Np * sizeof(double),
	                             (size_t)N * sizeof(double), N, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ONE call of a covariance fill launcher -- the launchers production calls, unchanged -- for the model the context holds
// (design, centred copy, covariance function, mode) into a host buffer of the caller's: the whole output region is
// uploaded, the launch runs, the whole region is downloaded, so that the caller's prefill shows what was and was not written.
//   GPEMU_FILL_STAGE  launch_cov_stage_batch as stage_matrices calls it (FILL_LOWER | FILL_IDENT_PAD): per matrix
//                     (Np + Rp + guard) rows of Np columns, the matrices that many rows apart
//   GPEMU_FILL_KVEC   M query rows to an Mp x Np block (Mp = M rounded up to 64), guard rows behind it
//   GPEMU_FILL_FULL   the 2-D launch_cov_fill with mode 0 as gpemu_cov_matrix runs it: Np x Np, guard rows behind it
// What the kernels may address is fixed by these shapes: lower tiles of rows [0, Np), rows [Np, Np + Rp) of a staged matrix,
// all of an Mp x Np or Np x Np block -- the footprint out_len has to cover, checked before anything runs.
// All device buffers are the call's own; of the context it reads the design (dX, dXg, dMid), the model's sizes, the mode
// and the schedule switches, and uses the stream.
extern "C" int gpemu_test_fill_launch(gpemu_ctx *ctx, const gpemu_fill_launch_args *p)
{
	if (!ctx || !p) return GPEMU_ERR_ARG;
	if (!ctx->dX) return fail(ctx, GPEMU_ERR_STATE, "model not set");
	if (p->op != GPEMU_FILL_STAGE && p->op != GPEMU_FILL_KVEC && p->op != GPEMU_FILL_FULL) return fail(ctx, GPEMU_ERR_ARG, "fill_launch: op");
	const bool stage = p->op == GPEMU_FILL_STAGE, kvec = p->op == GPEMU_FILL_KVEC;
	if (!p->thetas || !p->out || !p->form_out || !p->norm2_out || (stage && !p->rrows) || (kvec && !p->xq))
		return fail(ctx, GPEMU_ERR_ARG, "fill_launch: NULL pointer");
	if (p->nb < 1 || p->nb > GPEMU_MAX_BATCH || (!stage && p->nb != 1))
		return fail(ctx, GPEMU_ERR_ARG, "fill_launch: batch size must be 1..GPEMU_MAX_BATCH (1 for k-vectors and the full matrix)");
	if (p->form < -1 || p->form > (stage ? 2 : (kvec ? 1 : 0)) || (!stage && !kvec && p->form != 0))
		return fail(ctx, GPEMU_ERR_ARG, "fill_launch: form is -1/0/1/2 for the staging, -1/0/1 for k-vectors, 0 for the full matrix");
	if (kvec && p->M < 1) return fail(ctx, GPEMU_ERR_ARG, "fill_launch: M < 1");
	constexpr long ROWS_MAX = 1L << 20;
	if (p->guard < 0 || p->guard > ROWS_MAX || p->Rp < 0 || p->Rp > 4 * LEAF || p->M > ROWS_MAX)
		return fail(ctx, GPEMU_ERR_ARG, "fill_launch: guard, Rp or M out of range");
	const int nb = p->nb, nthetas = p->nthetas, N = ctx->N, d = ctx->d, Np = ctx->Np;
	if (nthetas < nthetas_for(ctx) || nthetas > GPEMU_MAX_PARAMS + 2) return fail(ctx, GPEMU_ERR_ARG, "fill_launch: nthetas");
	const int Rp = stage ? (p->Rp ? p->Rp : ctx->Rp) : 0, Mp = kvec ? round_up(p->M, LEAF) : 0;
	const long rows_each = (stage ? (long)Np + Rp : (kvec ? (long)Mp : (long)Np)) + p->guard;
	const long bstride = rows_each * Np, footprint = bstride * nb;
	// (the caller's rrows holds (nb - 1) * rstride + Rp * Np doubles: the stride is held to a few blocks so that a wrong one cannot ask for much)
	if (stage && (p->rstride < 0 || p->rstride > 4L * Rp * Np)) return fail(ctx, GPEMU_ERR_ARG, "fill_launch: rstride must be 0 .. 4 * Rp * Np");
	if (p->out_len < footprint) return fail(ctx, GPEMU_ERR_ARG, "fill_launch: the output buffer is shorter than the launch's footprint");
	std::vector<CovParams> ps((size_t)nb);
	for (int b = 0; b < nb; b++)
		if (const int rc = make_cov_params(ctx, p->thetas + (size_t)b * nthetas, nthetas, &ps[(size_t)b], p->norm2_out + b)) return rc;
	bool all_gram = ctx->dXg != nullptr;
	for (int b = 0; b < nb; b++) all_gram = all_gram && ps[(size_t)b].gram;
	if (p->form == 1 && (!all_gram || !ctx->dXg || !ctx->dMid))
		return fail(ctx, GPEMU_ERR_ARG, "fill_launch: the Gram form needs a centred design and hyper-parameters the admission rule accepts");
	if (p->form == 0)
		for (auto &q : ps) { q.gram = 0; q.cand_g = 0.0; }
	const bool gram_kernel = stage ? (p->form == 1 || (p->form == -1 && all_gram))
	                               : (kvec && (p->form == 1 || (p->form == -1 && ps[0].gram && ctx->sched.kvec_gram && ctx->dXg && ctx->dMid)));
	for (int b = 0; b < nb; b++)
		p->form_out[b] = stage ? ((gram_kernel || (ps[(size_t)b].gram && ctx->dXg)) ? 1 : 0) : (gram_kernel ? 1 : 0);

	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dOut, dRr, dQ;
	DevBuf<CovParams> dPp;
	const size_t rlen = stage ? (size_t)(nb - 1) * (size_t)p->rstride + (size_t)Rp * Np : 0;
	// every allocation first; from the first copy on nothing returns before the stream has been waited for (the copies read
	// ps, a vector of this frame, and the caller's buffers)
	HIPCHK(ctx, dOut.grow((size_t)footprint));
	if (stage) {
		HIPCHK(ctx, dRr.grow(rlen));
		HIPCHK(ctx, dPp.grow((size_t)nb));
	} else if (kvec)
		HIPCHK(ctx, dQ.grow((size_t)p->M * d));
	hipError_t e = hipMemcpyAsync(dOut, p->out, (size_t)footprint * 8, hipMemcpyHostToDevice, ctx->stream);
	if (stage) {
		if (e == hipSuccess) e = hipMemcpyAsync(dRr, p->rrows, rlen * 8, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(dPp, ps.data(), (size_t)nb * sizeof(CovParams), hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess)
			e = launch_cov_stage_batch(ctx->stream, dOut, Np, bstride, nb, ctx->dX, N, Np, d, dPp, FILL_LOWER | FILL_IDENT_PAD, dRr, Rp,
			                           ctx->dXg, gram_kernel, ctx->kind, p->rstride);
	} else if (kvec) {
		if (e == hipSuccess) e = hipMemcpyAsync(dQ, p->xq, (size_t)p->M * d * 8, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess)
			e = gram_kernel ? launch_cov_kvec_gram(ctx->stream, dOut, Np, dQ, p->M, Mp, ctx->dX, ctx->dXg, ctx->dMid, N, Np, d, ps[0])
			                : launch_cov_fill(ctx->stream, dOut, Np, dQ, p->M, Mp, ctx->dX, N, Np, d, ps[0], FILL_CLAMP);
	} else if (e == hipSuccess)
		e = launch_cov_fill(ctx->stream, dOut, Np, ctx->dX, N, Np, ctx->dX, N, Np, d, ps[0], 0);
	const hipError_t es = hipStreamSynchronize(ctx->stream);
	HIPCHK(ctx, e);
	HIPCHK(ctx, es);
	HIPCHK(ctx, hipMemcpyAsync(p->out, dOut, (size_t)footprint * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return GPEMU_OK;
}

// ONE call of a launcher that reads the device-resident factor -- the launchers the prediction products, gpemu_loo and
// gpemu_lgo call, unchanged -- on operands of the caller's, in device buffers of the call's own: every region the op takes is
// uploaded whole, the launch runs, every region is downloaded whole, so the caller's prefill shows what was read and what
// was written.  GPEMU_RES_LGO_TAIL runs lgo_chunk_tail (what lgo_run runs per chunk behind the staging launch) on the
// caller's staged matrices and returns what lgo_status makes of the info words, as gpemu_lgo does.
// What a launch may address is computed here first, from the kernels' grids and loops (kernels_linalg.hip), and anything
// beyond the given lengths is refused; the tables' entries are checked too, since the kernels index with them.
// No model is needed.  Of the context: the stream, and for the tail the schedule switches, the trace and the GEMM tile-table
// cache that every factorisation uses; prediction state, factorisation workspace and result ring are not touched.
extern "C" int gpemu_test_resident_launch(gpemu_ctx *ctx, const gpemu_resident_launch_args *p)
{
	if (!ctx || !p) return GPEMU_ERR_ARG;
	if (p->op < GPEMU_RES_SKINNY || p->op > GPEMU_RES_LGO_TAIL) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: op");
	constexpr long DIM_MAX = 1L << 16, LEN_MAX = 1L << 30;             // no product below leaves 63 bits
	const int op = p->op;
	const bool prod = op == GPEMU_RES_SKINNY || op == GPEMU_RES_GEMV, colsq = op == GPEMU_RES_LOO_COLSQ, loofin = op == GPEMU_RES_LOO_FINISH;
	const bool gather = op == GPEMU_RES_LGO_GATHER, stage = op == GPEMU_RES_LGO_STAGE, fin = op == GPEMU_RES_LGO_FINISH;
	const bool tail = op == GPEMU_RES_LGO_TAIL, lgo = gather || stage || fin || tail;
	// the double regions: host pointer, given length (uploaded and downloaded whole), the launch's footprint
	enum { R_LIN, R_KQ, R_VP, R_PART, R_BETAQ, R_Y, R_Z, R_T, R_RES, R_MEAN, R_VAR, R_WERR, R_STAT, R_COUNT };
	double *host[R_COUNT] = {};
	long len[R_COUNT] = {}, need[R_COUNT] = {};
	auto take = [&](int r, double *h, long given, long footprint) { host[r] = h; len[r] = given; need[r] = footprint; };
	const long N = p->N, Np = p->Np, ld = p->ld, nreg = p->nreg, bp = p->bp, nbc = p->nbc, g0 = p->g0, ngroups = p->ngroups;
	if (!prod) {
		const bool aug = !fin && !tail;                                 // the ops that read LinvAug: Np, ld (and nreg) are theirs
		if (N < 1 || N > DIM_MAX) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: N");
		if (aug && (N > Np || Np > DIM_MAX || Np % LEAF)) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: 1 <= N <= Np, Np a multiple of 64");
		if ((loofin || stage) && (nreg < 1 || nreg > 63)) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: nreg outside 1 .. 63");
		if (aug && (ld < Np || ld > DIM_MAX || (ld & 1))) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: ld must be even and >= Np");
	}
	if (lgo) {
		if (bp < LEAF || bp > 4096 || bp % LEAF || nbc < 1 || nbc > GPEMU_MAX_BATCH || g0 < 0 || ngroups > DIM_MAX || g0 + nbc > ngroups)
			return fail(ctx, GPEMU_ERR_ARG, "resident_launch: bp a multiple of 64 up to 4096, 1 <= nbc <= GPEMU_MAX_BATCH, 0 <= g0, g0 + nbc <= ngroups");
		if (!p->bsize || (gather ? !p->colrow : (!p->members || !p->moff))) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: NULL table");
		if (!gather && (p->nmembers < 1 || p->nmembers > DIM_MAX)) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: nmembers");
		for (long g = 0; g < ngroups; g++) {
			const long b = p->bsize[g];
			if (b < 1 || b > bp) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: a group size outside 1 .. bp");
			if (gather) continue;
			const long o = p->moff[g];
			if (o < 0 || o + b > p->nmembers) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: a group's members leave the table");
			for (long j = o; j < o + b; j++)
				if (p->members[j] < 0 || p->members[j] >= N) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: a member outside 0 .. N-1");
		}
		if (gather)
			for (long i = 0; i < N; i++)
				if (p->colrow[i] < -1 || p->colrow[i] >= ngroups * bp) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: a colrow entry outside -1 .. ngroups * bp - 1");
	}
	const long tmat = (2 * bp + LEAF) * bp, nmem = gather ? 0 : p->nmembers;
	if (stage || fin || tail) {
		if ((p->tstride & 1) || p->tstride < tmat || p->tstride > LEN_MAX) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: tstride must be even and >= (2 bp + 64) bp");
		take(R_T, p->t, p->t_len, (nbc - 1) * p->tstride + tmat);
	}
	if (prod) {
		const long K = p->K, ntot = p->ntot, ntri = p->ntri, nslice = p->nslice, klen = p->klen;
		if (K < 16 || K > DIM_MAX || K % 16 || ntot < LEAF || ntot > DIM_MAX || ntot % LEAF) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: K a multiple of 16, ntot a multiple of 64");
		if (ntri < 0 || ntri > ntot || ntri > K || ntri % 16) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: ntri a multiple of 16, at most ntot and K");
		if (nslice < 1 || nslice > 4096 || klen < 16 || klen > DIM_MAX || klen % 16) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: klen must be a multiple of 16");
		if (nslice * klen < K) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: the slices do not cover K");
		if (ld < K || ld > DIM_MAX || (ld & 3) || p->ldk < K || p->ldk > DIM_MAX || (p->ldk & 3))
			return fail(ctx, GPEMU_ERR_ARG, "resident_launch: ld and ldk must be multiples of 4 and >= K (32-byte row pieces)");
		if (p->ldv < ntot || p->ldv > DIM_MAX || p->vrows < 16 || p->vrows > DIM_MAX) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: ldv >= ntot, vrows >= 16");
		take(R_LIN, p->lin, p->lin_len, (ntot - 1) * ld + K);
		take(R_KQ, p->kq, p->kq_len, 15 * p->ldk + K);
		take(R_VP, p->vp, p->vp_len, nslice * p->vrows * p->ldv);
	} else if (colsq) {
		take(R_LIN, p->lin, p->lin_len, (N - 1) * ld + Np);
		take(R_PART, p->part, p->part_len, (long)loo_scratch_elems((int)N, (int)Np));
	} else if (loofin) {
		take(R_PART, p->part, p->part_len, (long)loo_scratch_elems((int)N, (int)Np));
		take(R_LIN, p->lin, p->lin_len, (Np + nreg) * ld + Np);
		take(R_BETAQ, p->betaq, nreg + nreg * nreg, nreg + nreg * nreg);
		take(R_Y, p->y, N, N);
		take(R_MEAN, p->mean, p->out_len, N);
		take(R_VAR, p->var, p->out_len, N);
	} else if (gather) {
		take(R_LIN, p->lin, p->lin_len, (N - 1) * ld + Np);
		take(R_Z, p->z, p->z_len, nbc * bp * Np);
	} else if (stage) {
		take(R_LIN, p->lin, p->lin_len, (Np + nreg) * ld + N);
		take(R_BETAQ, p->betaq, nreg + nreg * nreg, nreg + nreg * nreg);
	} else {
		if (fin) take(R_RES, p->res, 2 * nbc, 2 * nbc);
		take(R_Y, p->y, N, N);
		take(R_MEAN, p->mean, p->out_len, N);
		take(R_VAR, p->var, p->out_len, N);
		if (p->werr) take(R_WERR, p->werr, p->out_len, N);
		if (p->stat) take(R_STAT, p->stat, 3 * ngroups, 3 * ngroups);
		if (!p->info_out || (fin && !p->info)) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: NULL pointer");
	}
	for (int r = 0; r < R_COUNT; r++) {
		if (!need[r]) continue;
		if (!host[r]) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: NULL pointer");
		if (len[r] < need[r] || len[r] > LEN_MAX) return fail(ctx, GPEMU_ERR_ARG, "resident_launch: the launch would address memory beyond a region's length");
	}

	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<double> dev[R_COUNT], dPart;
	DevBuf<int> dTab, dInfo, dInfoOut;
	// every allocation first; from the first copy on nothing returns before the stream has been waited for
	for (int r = 0; r < R_COUNT; r++)
		if (need[r]) HIPCHK(ctx, dev[r].grow((size_t)len[r]));
	const size_t ntab = lgo ? (size_t)N + (size_t)nmem + 2 * (size_t)ngroups : 0;
	std::vector<int> tab(ntab, 0), inf(lgo ? (size_t)nbc : 1, INFO_NONE);
	const int *d_colrow = nullptr, *d_members = nullptr, *d_moff = nullptr, *d_bsize = nullptr;
	if (lgo) {
		int *h = tab.data();
		if (gather) memcpy(h, p->colrow, (size_t)N * sizeof(int));
		else { memcpy(h + N, p->members, (size_t)nmem * sizeof(int)); memcpy(h + N + nmem, p->moff, (size_t)ngroups * sizeof(int)); }
		memcpy(h + N + nmem + ngroups, p->bsize, (size_t)ngroups * sizeof(int));
		HIPCHK(ctx, dTab.grow(ntab));
		d_colrow = dTab; d_members = d_colrow + N; d_moff = d_members + nmem; d_bsize = d_moff + ngroups;
		if (fin || tail) {
			HIPCHK(ctx, dInfo.grow((size_t)nbc));
			HIPCHK(ctx, dInfoOut.grow((size_t)ngroups));
			if (fin) memcpy(inf.data(), p->info, (size_t)nbc * sizeof(int));
		}
		if (tail) HIPCHK(ctx, dPart.grow((size_t)nbc * (size_t)(bp / LEAF + 2)));
	}
	hipError_t e = hipSuccess;
	int rc = GPEMU_OK;
	for (int r = 0; r < R_COUNT && e == hipSuccess; r++)
		if (need[r]) e = hipMemcpyAsync(dev[r], host[r], (size_t)len[r] * 8, hipMemcpyHostToDevice, ctx->stream);
	if (lgo && e == hipSuccess) e = hipMemcpyAsync(dTab, tab.data(), ntab * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
	if ((fin || tail) && e == hipSuccess) e = hipMemcpyAsync(dInfo, inf.data(), (size_t)nbc * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
	if ((fin || tail) && e == hipSuccess) e = hipMemcpyAsync(dInfoOut, p->info_out, (size_t)ngroups * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) {
		hipStream_t s = ctx->stream;
		if (op == GPEMU_RES_SKINNY)
			e = launch_skinny_nt(s, dev[R_KQ], p->ldk, dev[R_LIN], ld, dev[R_VP], p->ldv, (long)p->vrows * p->ldv, 1, p->ntot, p->K, p->ntri, p->nslice, p->klen);
		else if (op == GPEMU_RES_GEMV)
			e = launch_gemv_tri(s, dev[R_KQ], p->ldk, dev[R_LIN], ld, dev[R_VP], p->ldv, (long)p->vrows * p->ldv, 1, p->ntot, p->K, p->ntri, p->nslice, p->klen);
		else if (colsq) e = launch_loo_colsq(s, dev[R_LIN], ld, (int)N, (int)Np, dev[R_PART]);
		else if (loofin) e = launch_loo_finish(s, dev[R_PART], dev[R_LIN], ld, (int)N, (int)Np, (int)nreg, dev[R_BETAQ], dev[R_Y], dev[R_MEAN], dev[R_VAR]);
		else if (gather) e = launch_lgo_gather(s, dev[R_LIN], ld, (int)N, (int)Np, d_colrow, d_bsize, (int)g0, (int)nbc, (int)bp, dev[R_Z]);
		else if (stage)
			e = launch_lgo_stage(s, dev[R_T], p->tstride, (int)g0, (int)nbc, (int)bp, d_members, d_moff, d_bsize, dev[R_LIN], ld, (int)Np, (int)nreg, dev[R_BETAQ]);
		else if (fin)
			e = launch_lgo_finish(s, dev[R_T], p->tstride, (int)nbc, (int)bp, d_members, d_moff, d_bsize, dInfo, dev[R_RES], dev[R_Y], (int)g0, (int)ngroups,
			                      dev[R_MEAN], dev[R_VAR], need[R_WERR] ? (double *)dev[R_WERR] : nullptr, need[R_STAT] ? (double *)dev[R_STAT] : nullptr, dInfoOut);
		else
			rc = lgo_chunk_tail(ctx, dev[R_T], p->tstride, (int)nbc, (int)bp, dInfo, dPart, d_members, d_moff, d_bsize, dev[R_Y], (int)g0, (int)ngroups,
			                    dev[R_MEAN], dev[R_VAR], need[R_WERR] ? (double *)dev[R_WERR] : nullptr, need[R_STAT] ? (double *)dev[R_STAT] : nullptr, dInfoOut);
	}
	const hipError_t es = hipStreamSynchronize(ctx->stream);
	if (rc) return rc;
	HIPCHK(ctx, e);
	HIPCHK(ctx, es);
	for (int r = 0; r < R_COUNT; r++)
		if (need[r]) HIPCHK(ctx, hipMemcpyAsync(host[r], dev[r], (size_t)len[r] * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (fin || tail) HIPCHK(ctx, hipMemcpyAsync(p->info_out, dInfoOut, (size_t)ngroups * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return tail ? lgo_status(ctx, (int)nbc, p->info_out + g0) : GPEMU_OK;
}

// the GEMM tile order of a launch with tiles_m x tiles_n tiles (tri: lower triangle only) and super-blocks of side sb:
// pure host logic, no device needed.  Returns the table length; fills out[0 .. min(len, cap)).
extern "C" int gpemu_test_tile_table(int tiles_m, int tiles_n, int tri, int sb, int *out, int cap)
{
	if (tiles_m < 1 || tiles_n < 1 || tiles_m > 32767 || tiles_n > 32767 || sb < 1) return -GPEMU_ERR_ARG;
	const std::vector<int> t = gpemu::build_tile_table(tiles_m, tiles_n, tri, sb);
	if (out)
		for (int i = 0; i < (int)t.size() && i < cap; i++) out[i] = t[i];
	return (int)t.size();
}

/* the row table of the square product with row-start skipping (gpemu::build_row_table): same hook, same conventions */
extern "C" int gpemu_test_row_table(int tiles_m, int bm, int kstart_off, int k0, int k1, int *out, int cap)
{
	if (tiles_m < 1 || tiles_m > 32767 || bm < 16 || k1 <= k0) return -GPEMU_ERR_ARG;
	const std::vector<int> t = gpemu::build_row_table(tiles_m, bm, kstart_off, k0, k1);
	if (out)
		for (int i = 0; i < (int)t.size() && i < cap; i++) out[i] = t[i];
	return (int)t.size();
}

namespace gpemu { hipError_t launch_fill_random(hipStream_t s, double *p, size_t n, unsigned seed); }

// times `reps` launches of one GEMM shape with HIP events on the ctx stream (device-resident random operands)
extern "C" int gpemu_test_gemm_bench(gpemu_ctx *ctx, int m, int n, int k, int ld_in, int cfg, int tri, int beta,
                                     int reps, double *ms_avg, double *flops)
{
	if (!ctx || m < 1 || n < 1 || k < 16 || (k % GEMM_BK) != 0 || reps < 1 || (cfg != 0 && cfg != 2 && cfg != 8)) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const long ld = std::max(std::max(k, n), ld_in);
	DevBuf<double> da, dc;
	const size_t rows = (size_t)std::max(m, n);
	HIPCHK(ctx, da.grow(rows * ld));
	HIPCHK(ctx, dc.grow((size_t)m * ld));
	HIPCHK(ctx, launch_fill_random(ctx->stream, da, rows * ld, 1u));
	HIPCHK(ctx, launch_fill_random(ctx->stream, dc, (size_t)m * ld, 2u));
	if (getenv("GPEMU_BENCH_ZERO")) {      // zero operands: the clock-limited ceiling (no data-dependent switching power)
		HIPCHK(ctx, hipMemsetAsync(da, 0, rows * ld * 8, ctx->stream));
		HIPCHK(ctx, hipMemsetAsync(dc, 0, (size_t)m * ld * 8, ctx->stream));
	}
	GemmArgs g{};
	g.C = dc; g.A = da; g.B = da; g.ldc = ld; g.lda = ld; g.ldb = ld; g.m = m; g.n = n; g.k0 = 0; g.k1 = k;
	g.alpha = -1.0; g.beta = beta; g.tri = tri;
	if (getenv("GPEMU_BENCH_LD0")) { g.lda = 0; g.ldb = 0; }   // every operand row aliases row 0: staging loads always hit L1/L2
	ctx->trace_next = 0; ctx->trace_tag.clear();
	HIPCHK(ctx, trace_clear(ctx));
	g.trace = trace_slot(ctx, "gemm_bench m=%d n=%d k=%d", m, n, k);   // (nullptr when tracing is off)
	g.force_cfg = cfg;                                      // 2: 64x64 tiles, 8: 128x128 tiles, 0: the automatic choice
	apply_sched(ctx->sched, g);
	hipEvent_t e0, e1;
	hipEventCreate(&e0); hipEventCreate(&e1);
	hipError_t e = launch_gemm(ctx->stream, g);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	hipEventRecord(e0, ctx->stream);
	for (int r = 0; r < reps && e == hipSuccess; r++) e = launch_gemm(ctx->stream, g);
	hipEventRecord(e1, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	float ms = 0.f;
	hipEventElapsedTime(&ms, e0, e1);
	hipEventDestroy(e0); hipEventDestroy(e1);
	HIPCHK(ctx, e);
	if (ms_avg) *ms_avg = ms / reps;
	if (flops) *flops = gemm_flops(g);
	return GPEMU_OK;
}

extern "C" int gpemu_test_potrf(gpemu_ctx *ctx, int n, double *a, int *info)
{
	if (!ctx || n < 1 || !a) return GPEMU_ERR_ARG;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const int Np = round_up(n, LEAF), Rp = 64;
	std::vector<double> h((size_t)(Np + Rp) * Np, 0.0);
	for (int i = 0; i < Np; i++)
		for (int j = 0; j <= i; j++)
			h[(size_t)i * Np + j] = (i < n) ? a[(size_t)i * n + j] : (i == j ? 1.0 : 0.0);
	DevBuf<double> dT;
	DevBuf<int> dInfo;
	HIPCHK(ctx, dT.grow(h.size()));
	HIPCHK(ctx, dInfo.grow(1));
	const Tall t{dT, dInfo, Np, Rp, 1, (long)h.size()};
	int big = INFO_NONE, inf = 0;
	HIPCHK(ctx, trace_clear(ctx));
	HIPCHK(ctx, hipMemcpyAsync(dT, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dInfo, &big, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, potrf_all(ctx, t, 0));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(h.data(), dT, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(&inf, dInfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if (info) *info = pivot_info(inf);
	for (int i = 0; i < n; i++)
		for (int j = 0; j < n; j++) a[(size_t)i * n + j] = (j <= i) ? h[(size_t)i * Np + j] : 0.0;
	return GPEMU_OK;
}
