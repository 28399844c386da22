// gpemu_internal.hpp -- shared declarations of the gfx950 device library.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include <map>
#include <set>
#include <tuple>

#include "gpemu.h"

namespace gpemu {

constexpr int LEAF = 64;          // diagonal block / padding granule
constexpr int GEMM_BM = 128;
constexpr int GEMM_BN = 128;
constexpr int GEMM_BK = 16;
constexpr int JOINT_RHS = 64;     // right-hand-side rows of the joint factor's tall matrix: the most observation rows of a call

inline int round_up(int x, int m) { return ((x + m - 1) / m) * m; }

// Covariance parameters handed to kernels by value.
// pow-exp (emulator.c:101-152): amp = exp(t0), nug = exp(t1), w[k] = sqrt(0.5)/exp(t_{k+2}) (coordinate scale:
//   exponent = -sum ((x_k-y_k) w_k)^2), eps = 1e-10
// Matern  (emulator.c:344-386, 438-480): amp = t0, nug = t1, w[0] = 1/exp(t2) (all coordinates), eps = 1e-16
// cand: upper bound of sum ((x_k-y_k) w_k)^2 over pairs with every |x_k-y_k| < eps (plus rounding slack); only
//   those pairs run the exact per-coordinate "same point" test of the nugget rule.
struct CovParams {
	int kind;
	int d;
	double amp;
	double nug;
	double eps;
	double cand;
	int gram;            // 1: the square training fill may use the MFMA Gram form of the squared distances (kernels_cov.hip)
	int pad_;
	double cand_g;       // Gram form: squared scaled distances at or below this are recomputed from differences
	double cand_w;       // the exact gradient's Gram-form weights (any length scale): likewise, with that form's own error bound
	double w[GPEMU_MAX_PARAMS];
};

// The box and the two contexts' squared inverse lengths s_l = exp(-2 theta_{2+l}) of a sensitivity call, handed to its
// prep kernel by value (kernels_sens.hip); SENS_CST: rows of the per-coordinate constants that kernel leaves for the sweep
// kind[l]: the input measure of coordinate l (GPEMU_MEASURE_*: for a Gaussian one lo is the mean and hi the standard
// deviation); meas: 0 every coordinate uniform, 1 every coordinate Gaussian, 2 both kinds (the sweeps' MEAS parameter)
struct SensBox {
	int d;
	int meas;
	double s[GPEMU_MAX_PARAMS], t[GPEMU_MAX_PARAMS];
	double lo[GPEMU_MAX_PARAMS], hi[GPEMU_MAX_PARAMS];
	int kind[GPEMU_MAX_PARAMS];
};
// rows 0 .. SENS_CST - 1 are what a sweep's pair factor reads (the all-uniform and the all-Gaussian sweep stage these alone),
// row SENS_CST_KIND the coordinate's kind (0.0 / 1.0; the mixed sweep stages it too), row SENS_CST_S the squared inverse
// length s of context a itself (the one-context finishes of a Gaussian coordinate: row 0 no longer holds s / 2 there)
constexpr int SENS_CST = 7;
constexpr int SENS_CST_KIND = 7, SENS_CST_S = 8, SENS_CST_ROWS = 9;

// C[m x n] = beta*C + alpha * A[m x K] * B[n x K]^T over k in [k0,k1)
struct GemmArgs {
	double *C;
	const double *A;
	const double *B;
	long ldc, lda, ldb;
	int m, n;
	int k0, k1;          // multiples of GEMM_BK
	double alpha;
	int beta;            // 0 or 1
	int tri;             // 1: skip tiles with tn*BN > tm*BM + BM-1 + diag_off
	int diag_off;
	int kstart_mode;     // 1: k starts at max(k0, floor_BK(tm*BM - kstart_off))   (upper-triangular A rows)
	int kstart_off;
	int kend_mode;       // 1: k ends at min(k1, ceil_BK(tn*BN + BN - kend_off))   (lower-triangular B rows)
	int kend_off;
	long bsC, bsA, bsB;  // element strides between the matrices of a batch (grid.y = nbatch)
	int nbatch;          // 0/1: single problem
	int ksplit;          // > 1: grid.y = k-slices of ONE problem; slice s takes k in [k0 + s*klen, k0 + (s+1)*klen) and
	                     // writes its partial product to C + s*bsC (beta = 0); the consumer sums the slices in order
	int order_mode;      // 2: dense enumeration of the lower-triangular tiles, 3: tile table (set by launch_gemm)
	const int *tile_table; // order_mode 3: entry blockIdx.x = (tm << 16) | tn, or -1 for none
	unsigned long long *trace;   // optional {first start, last end} device timestamps of this launch (GPEMU_TRACE)
	int fa;              // factor-ahead: the workgroup of tile (0,0) factors its updated 64x64 diagonal block (64x64 tiles only)
	int fa_c0;           // global column of that block (for the 1-based index of a failed pivot)
	int *fa_info;        // info words (one per matrix of the batch)
	// schedule switches of the calling context (Sched below), carried per call: nothing process-wide
	int big_tiles;       // 128x128 tiles once a lock-step launch has this many of them (0: 1024)
	int table_sb;        // XCD-blocked tile table for launches of >= 512 tiles: side of the super-blocks (0: off)
	int force_cfg;       // test/bench hook: 2 = 64x64 tiles, 8 = 128x128 tiles, 0 = automatic
	int keep_idle_waves; // 1: waves above the diagonal of a triangular update's diagonal tiles compute their (unread) output anyway (A/B switch)
	int no_neg_modifier; // 1: alpha = -1 by negating the accumulators on the way in and out, as rounds 1-3 did (A/B switch)
	int row_table;       // 1: the square product with row-start skipping (C^-1 = U U^T) gives whole tile rows to an XCD (build_row_table)
	int stagger_ticks;   // > 0: of the launch's first round, the workgroup in the odd slot of its CU starts this many 10 ns ticks late (kernel comment)
	// riders (128x128 tiles of a triangular update, C - A B^T): the two idle waves of every diagonal tile update the
	// ride_rows x 128 block of right-hand-side rows over their tile column from the B image in LDS (kernel comment)
	double *ride_C;      // row 0 of the right-hand-side block, at column 0 of the update (ldc, bsC as C)
	const double *ride_A; // the same rows at column 0 of the panel (lda, bsA as A)
	int ride_rows;       // 16 or 0
};

// what a lock-step factorisation works on: nb tall matrices, stride elements apart, and their info words (a view, no owner)
// rhs_live: how many of the Rp right-hand-side rows can be non-zero (the rest are +0 and stay +0); 0: the view cannot say
struct Tall { double *T; int *info; int Np, Rp, nb; long stride; int rhs_live; };

// Schedule switches of ONE context: read from the environment once, when the context is created (INTEGRATION.md lists
// the variables), and constant for its lifetime.  Two contexts of a process may differ; nothing process-wide is written
// after start-up, so contexts created and driven from several host threads (csrc/host/multi.c) cannot disturb each other,
// and a context's cached launch graphs always match its switches.
struct Sched {
	int gemm_big_tiles = 1024;   // GPEMU_GEMM_BIG_TILES
	int gemm_table = 8;          // GPEMU_GEMM_TABLE (0 .. 64)
	int factor_ahead = 1;        // GPEMU_FACTOR_AHEAD: the update's tile (0,0) factors the next diagonal block
	int fill_gram = 1;           // GPEMU_FILL_GRAM: MFMA Gram form of the training fill
	int kvec_gram = 1;           // GPEMU_KVEC_GRAM: MFMA Gram form of the prediction sweep's k-vectors
	int gemv_point = 1;          // GPEMU_GEMV_POINT: ONE query takes the matrix-vector kernel instead of the skinny MFMA product
	int idle_waves = 1;          // GPEMU_IDLE_WAVES: waves wholly above the diagonal of a diagonal tile issue no matrix instructions
	int nb_top = 0;              // GPEMU_NB_TOP: outer panel width; 0 = automatic (512 for one matrix, 2048 / 1024 for a batch)
	int split_rhs_rows = 1;      // GPEMU_SPLIT_RHS_ROWS: big-tile updates take the 64 right-hand-side rows in a launch of their own
	int rhs_ride = 1;            // GPEMU_RHS_RIDE: in those updates the live right-hand-side rows (at most 16) ride in the idle waves of the diagonal tiles instead
	int neg_modifier = 1;        // GPEMU_NEG_MODIFIER: C - A B^T through the NEG bit of the fp64 matrix instruction
	int grad_gram = 1;           // GPEMU_GRAD_GRAM: the exact gradient's tile distances from the matrix unit (grad_exact_gram_kernel)
	int leaf_staged = -1;        // GPEMU_LEAF_STAGED: the leaf solve moves whole 512-byte row pieces through an LDS strip (1), element-wise (0), automatic by launch size (-1)
	int diag_inv_ahead = 1;      // GPEMU_DIAG_INV_AHEAD: the leaf solve takes the 16x16 diagonal inverses the factoring workgroup left in the block's upper part (0: every workgroup computes them)
	int leaf_pair = 1;           // GPEMU_LEAF_PAIR: first block of a 128-column pair in one launch (leaf solve + K=64 update, leaf_pair_kernel); 0: two launches
	int corner_row_table = 1;    // GPEMU_CORNER_ROW_TABLE: C^-1 = U U^T with whole tile rows per XCD (0: row-major enumeration, round-robin over the XCDs)
	int stagger_us = 20;         // GPEMU_STAGGER_US: first-round offset between the two workgroups of a CU in the 128x128 GEMM (0 = none)
	int panel_rows = 1;          // GPEMU_PANEL_ROWS: the rows under a 256-column group's cut in one pass (panel_rows_kernel): 0 never, 1 lock-step batches by launch size, 2 always
	int panel_split = 1;         // GPEMU_PANEL_SPLIT: the cut: k > 0 = 64 k rows under the group (1 measured best), 0 = the end of the outer panel's diagonal square
	int target_panel = 2048;     // GPEMU_TARGET_PANEL: target columns per panel of U_q U_t^T in gpemu_design_target_gain, a multiple of 64 (the bits do not depend on it)
};

// The one owner of device or pinned host memory in this library: move-only, released by the destructor, knows its element
// count.  grow() is a compare when the capacity suffices; otherwise it releases and allocates afresh (contents are NOT
// kept), and after a failed allocation the buffer is empty.  Reads as the plain pointer it holds.  Work that may still use
// a context's buffer is waited for by the context's grow() (gpemu_api.hip), not here.
struct DeviceMem {
	static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
	static hipError_t release(void *p) { return hipFree(p); }
};
struct PinnedMem {
	static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
	static hipError_t release(void *p) { return hipHostFree(p); }
};

template <class T, class Mem>
class Buf {
	T *p_ = nullptr;
	size_t n_ = 0;
public:
	Buf() = default;
	Buf(Buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
	Buf &operator=(Buf &&o) noexcept
	{
		if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
		return *this;
	}
	~Buf() { reset(); }
	operator T *() const { return p_; }
	size_t size() const { return n_; }
	void reset()
	{
		if (p_) (void)Mem::release(p_);
		p_ = nullptr; n_ = 0;
	}
	hipError_t grow(size_t n)
	{
		if (n <= n_) return hipSuccess;
		reset();
		const hipError_t e = Mem::alloc((void **)&p_, n * sizeof(T));
		if (e != hipSuccess) { p_ = nullptr; return e; }
		n_ = n;
		return hipSuccess;
	}
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

struct ProfState {
	int cls = GPEMU_PROF_NONE;
	std::vector<hipEvent_t> ev;   // pairs
	double flops = 0, bytes = 0;
	int n = 0;
	std::vector<std::string> tag;  // one label per launch (GPEMU_PROF_DUMP=1 prints them with their times)
};

// One entry of the result ring: the results of an enqueued batch stay readable while the next RES_RING - 1 are enqueued.
struct ResSlot {
	hipEvent_t ev = nullptr;     // recorded behind the copies into the slot
	int nb = 0;                  // batch size; 0: nothing collectable here
	int kind = 0;                // 0: likelihood batch, 1: value+gradient batch
	std::vector<double> th;      // value+gradient batches: the thetas they were enqueued with (theta[0] = 0)
	int nthetas = 0;
	int mode = 0;                // the context's mode flags when the batch was enqueued
	double *res = nullptr;       // the slot's part of the three pinned rings (set by ensure_batch_slots):
	int *info = nullptr;         //   nb x res_len results, nb info words,
	double *grad = nullptr;      //   nb x GRAD_NP_MAX gradient sums
};

// Pinned upload ring of the hyper-parameters: an entry is reused once the copies out of it have executed.
struct ParamRing {
	static constexpr unsigned RING = 4;
	PinnedBuf<CovParams> params;     // RING x GPEMU_MAX_BATCH
	PinnedBuf<double> gph;           // the length thetas of value+gradient batches: RING x GPEMU_MAX_BATCH x GPEMU_MAX_PARAMS
	hipEvent_t ev[RING] = {};        // recorded behind the copies out of an entry
	unsigned next = 0;
	unsigned slot = 0;               // entry of the batch being enqueued
};

// The host-buffer prediction entries (gpemu_predict_batch, _mean, _mean_grad, _var_grad and their halves) and the one batch a
// context can have enqueued through any of them: its kind and its number of queries.  PRED_NONE: nothing pending.
enum PredKind { PRED_NONE = 0, PRED_MEAN_VAR, PRED_MEAN, PRED_MEAN_GRAD, PRED_VAR_GRAD };
struct PredPending {
	PredKind kind = PRED_NONE;
	int M = 0;
};

// The ensemble sampler's state on a context (gpemu_sample_* / gpemu_calib_sample): the owner of everything
// those entries keep.  prior: the per-coordinate table of gpemu_sample_set_prior (kernels_sample.hip has its layout; prior_d > 0:
// set), independent of the model as the calibration table is.  The rest belongs to gpemu_calib_sample, sized by the call's
// shape (W, d, nr, trace records of a chunk) and reused while it fits: x, lp, nacc the ensemble; y, aux a half-step's proposals;
// mean, var (nr rows of W / 2), stat, worst its evaluation; trx, trlp the staged trace records; ev_obs: the component streams
// behind the proposal, ev_comp[c]: this stream behind component c's sweep.  chunk_records: the test hook's bound (0: default).
struct SampleState {
	int prior_d = 0;
	DevBuf<double> prior;
	DevBuf<double> x, lp, y, aux, mean, var, stat, trx, trlp;
	DevBuf<int> nacc, worst;
	hipEvent_t ev_obs = nullptr;
	std::vector<hipEvent_t> ev_comp;
	int chunk_records = 0;
	SampleState() = default;
	SampleState(const SampleState &) = delete;
	SampleState &operator=(const SampleState &) = delete;
	// the run's buffers and events (the caller has waited for the stream); the prior stays
	void release_run()
	{
		for (auto *b : {&x, &lp, &y, &aux, &mean, &var, &stat, &trx, &trlp}) b->reset();
		nacc.reset(); worst.reset();
		if (ev_obs) (void)hipEventDestroy(ev_obs);
		for (auto e : ev_comp) (void)hipEventDestroy(e);
		ev_obs = nullptr;
		ev_comp.clear();
	}
	void release() { release_run(); prior.reset(); prior_d = 0; }
	~SampleState() { release(); }
};

} // namespace gpemu

struct gpemu_ctx {
	~gpemu_ctx();                      // waits for the stream, then releases everything (gpemu_api.hip)
	int device = 0;
	hipStream_t stream = nullptr;      // the context's one stream: every launch and copy of the context is ordered on it
	gpemu::Sched sched;                // schedule switches, fixed at creation
	std::string err;

	// model
	int kind = 0, order = 0, N = 0, d = 0, nreg = 0, nrhs = 0;
	int Np = 0, Rp = 0;
	gpemu::DevBuf<double> dX;    // N x d
	gpemu::DevBuf<double> dXg;   // N x d, centred per dimension (x - mid_k): operands of the Gram-form fill
	gpemu::DevBuf<double> dMid;  // d: the centres mid_k (the Gram-form k-vectors centre their query rows with them)
	std::vector<double> xhalf;   // d: half range of each design coordinate
	gpemu::DevBuf<double> dY;    // N
	gpemu::DevBuf<double> dRrows; // Rp x Np : row 0 = y, rows 1..nreg = H columns, zero padded
	std::vector<double> hX, hY;

	// factorisation workspace: tall matrix T (all matrices of a batch together)
	gpemu::DevBuf<double> dT;
	int nb = 1;                  // matrices factored in lock-step by the current / last factorisation
	size_t T_stride = 0;         // elements between consecutive matrices of the batch
	gpemu::DevBuf<double> dGramPart; // batch_cap() x [Np/64][Rp*Rp]: sized by model and batch, gone with the model

	// per-matrix result slots, sized by the largest batch so far and kept across models (ensure_batch_slots)
	gpemu::DevBuf<double> dRes;  // per matrix: Rp*Rp gram + logdet + spare
	static constexpr int RES_RING = 4;
	static constexpr int GRAD_NP_MAX = 2 * GPEMU_MAX_PARAMS + 2;   // reduced gradient sums per batch element
	gpemu::PinnedBuf<double> hResRing;  // RES_RING x batch_cap() x res_len
	gpemu::PinnedBuf<int> hInfoRing;    // RES_RING x batch_cap()
	gpemu::DevBuf<double> dGradSum;     // batch_cap() x GRAD_NP_MAX
	gpemu::PinnedBuf<double> hGradRing; // RES_RING x batch_cap() x GRAD_NP_MAX
	gpemu::DevBuf<int> dInfo;           // batch_cap() info words
	int batch_cap() const { return (int)dInfo.size(); }   // (dInfo is allocated last: its size says that all of them are there)
	gpemu::ResSlot ring[RES_RING];
	unsigned long long res_seq = 0;     // batches enqueued since the ring was (re)allocated
	gpemu::ResSlot &newest() { return ring[(res_seq + RES_RING - 1) % RES_RING]; }
	gpemu::ParamRing pring;
	size_t res_len = 0;

	// cached launch graphs for potrf, keyed by (Np, Rp, with_inverse, nb)
	using GraphKey = std::tuple<int, int, int, int>;
	std::map<GraphKey, hipGraphExec_t> graphs;
	std::set<GraphKey> warm;     // shapes factored once with plain launches (the graph is recorded on the second call)
	bool use_graph = true;

	// prediction state
	bool pred_ready = false;
	gpemu::DevBuf<double> dLinvAug;  // (Np + Rp) x Np : rows [0,Np) = L^-1, row Np = gamma, rows Np+1.. = W^T
	gpemu::DevBuf<double> dBetaQ;    // beta (nreg) then Q (nreg*nreg)
	double kappa = 0;
	gpemu::CovParams pred_cov;
	std::vector<double> h_beta, h_Q;
	gpemu::DevBuf<double> dKq, dV;   // batch buffers
	// staging of the host-buffer entries of every kind, stage_cap() queries: dXq coordinates; dMean means, then variances (one
	// allocation: a small batch comes back in ONE copy); hStage pinned, coordinates, then means, then variances
	gpemu::DevBuf<double> dXq, dMean;
	gpemu::PinnedBuf<double> hStage;
	size_t stage_cap() const { return hStage.size() / (size_t)(d + 2); }   // (hStage is allocated last, and gone with the model)
	double *dVar() const { return dMean + stage_cap(); }
	gpemu::PredPending pred_pending;  // the enqueued, not yet collected prediction batch; gone with the model (free_model)
	gpemu::DevBuf<double> dMeanPart;  // mean-only sweep: slice partial sums, predict_mean_slices(Np) x queries of a block
	// mean-gradient sweep (gpemu_predict_mean_grad): its own scratch and staging.  dMGradPart: per slice and query of a block
	// the mean's partial sum, then predict_mean_grad_width(d) gradient sums; dMGrad / hMGrad: mgrad_cap() x d gradients
	// (dMGrad / hMGrad also stage the gradients of the variance-gradient entry's host forms: one batch is pending at a time)
	gpemu::DevBuf<double> dMGradPart, dMGrad;
	gpemu::PinnedBuf<double> hMGrad;
	size_t mgrad_cap() const { return d ? hMGrad.size() / (size_t)d : 0; }
	// variance-gradient entry (gpemu_predict_var_grad).  dLinvAugT: dLinvAug transposed, Np x (Np + Rp), made by
	// the first call after a set-up (linvT_ready; cleared with pred_ready); dVGradPart: per slice and query of a block
	// predict_mean_grad_width(d) gradient sums, then two rows of scratch for a mean or variance the caller did not ask for.
	// The entry also uses dKq and dV, as gpemu_predict_batch does.
	bool linvT_ready = false;
	gpemu::DevBuf<double> dLinvAugT, dVGradPart;
	// joint-covariance entry (gpemu_predict_cov).  dCovR: the r rows of a call (M' x Rp, M' = M rounded up to 64),
	// then two rows of M' for a mean the caller did not ask for and the variance nobody reads; dCov: the M x M result of the
	// host-buffer entry before it is copied out.  The entry also uses dKq and dV, as gpemu_predict_batch does.
	gpemu::DevBuf<double> dCovR, dCov;
	// hold-out validation and joint draws (gpemu_predict_joint_factor / _draw).  dJoint: the tall matrix
	// [S ; 64 right-hand-side rows], (Mp + 64) x Mp with Mp = joint_M rounded up to 64 -- after a factor call the plain lower
	// factor L_S, zeros above the diagonal; dJointMean: the means of its queries (Mp); joint_M > 0: both are resident and belong
	// to the prediction state (cleared with pred_ready).  dJointPart: the Gram partials of the solved rows, then the finished
	// Gram matrix and the log determinant; dJointZ: the zero-padded normals of a block of draws; dJointIO / dJointInfo: the
	// host entries' device copies of noise, yobs, var, werr, the statistics, z and out, and their info word.
	int joint_M = 0;
	gpemu::DevBuf<double> dJoint, dJointMean, dJointPart, dJointZ, dJointIO;
	gpemu::DevBuf<int> dJointInfo;
	bool cinv_ready = false;
	bool fact_in_T = false;      // the factorisation (with inverse rows) behind the prediction state sits in THIS context's workspace, element 0
	                             // (false after gpemu_predict_setup_batch for every context but the first: their factorisations ran in the first one's)
	// leave-one-out (gpemu_loo): partial column sums; means then variances (N each) on the device and in pinned memory
	gpemu::DevBuf<double> dLooPart, dLoo;
	gpemu::PinnedBuf<double> hLoo;
	// leave-group-out (gpemu_lgo), per chunk of nbc groups padded to bp: dLgoZ the gathered columns of L^-1 as
	// rows (nbc x bp x Np), dLgoT the tall matrices [P_BB ; 64 right-hand-side rows ; identity rows] (nbc x (2 bp + 64) x bp),
	// dLgoPart the partial sums of |w|^2 then {maha, 2 sum log R_ii} per group, dLgoInfo the factorisation's info words;
	// dLgoTab / hLgoTab the index tables of a call (device / pinned; lgo_ev: recorded behind the upload); dLgoOut / dLgoInfoOut
	// the host entry's results before they are copied out
	gpemu::DevBuf<double> dLgoZ, dLgoT, dLgoPart, dLgoOut;
	gpemu::DevBuf<int> dLgoTab, dLgoInfo, dLgoInfoOut;
	gpemu::PinnedBuf<int> hLgoTab;
	hipEvent_t lgo_ev = nullptr;
	// sensitivity entries (gpemu_sens_cov / gpemu_sens_main): dSensPrep the per-point tables of both contexts
	// (2 x 5 x d x N), dSensCst the sweep's per-coordinate constants, dSensPart the tiles' partial sums, dSensOut the 3 + 2 d
	// results of the host entry (and E0 of the main-effect entry), dSensGrid that entry's grid, then its curves; sens_ev: this
	// context's stream behind the other context's pending work, sens_ev2: the other's stream behind this call
	gpemu::DevBuf<double> dSensPrep, dSensCst, dSensPart, dSensOut, dSensGrid;
	// gpemu_sens_post: dSensP the pair weights P = C^-1 - W Q W^T on the lower tiles (Np x Np), dSensG = W Q
	// (N x nreg), dSensPostPart the weighted sweep's partial sums; sens_post_N: the N they were last written for (0: never)
	gpemu::DevBuf<double> dSensP, dSensG, dSensPostPart;
	int sens_post_N = 0;
	// second order: dSensPex2 the leave-two-out products of both contexts (2 x npairs x N), dSensPairPart the
	// pair sweeps' partial sums (npairs per tile), dSensPairOut the npairs results of the host entries
	gpemu::DevBuf<double> dSensPex2, dSensPairPart, dSensPairOut;
	hipEvent_t sens_ev = nullptr, sens_ev2 = nullptr;
	// expected IMSE reduction of candidate runs (gpemu_design_gain).  dDesignKH: [K ; HK], (Np + 64) x Np, and
	// dDesignHm (64 x 64), kept between calls: design_serial / design_box say which set-up (pred_serial), box and kinds they
	// were built for (0: none).  Per block of candidates: dDesignPrepQ the candidates' own tables, dDesignA the rows of a
	// (mb' x Np), dDesignT = a [K | HK] (mb' x (Np + 64)), dDesignR the r rows, dDesignB the b rows (64 each), dDesignPart the
	// cross sweep's partials; dDesignOut gain, num, var of the host entry; design_mb: the candidates of the last block (0: none)
	gpemu::DevBuf<double> dDesignKH, dDesignHm, dDesignPrepQ, dDesignA, dDesignT, dDesignR, dDesignB, dDesignPart, dDesignOut;
	unsigned long long pred_serial = 0, design_serial = 0;   // pred_serial: counts the prediction set-ups of this context
	gpemu::SensBox design_box{};
	int design_mb = 0;
	// greedy batches (gpemu_design_batch), beside the block above: dBatchW the rows of w (mb' x Np), dBatchLam and
	// dBatchMu (mb x nbatch), dBatchE (256 x 256), dBatchSv what the gather lays out of a pick, dBatchDots the column kernel's four
	// dots, dBatchSt v_S, num_S and gain (3 x mb); on ctxs[0] also dBatchTab (the contexts' gain pointers, the weights, the picked
	// marks) and dBatchIO (the host entry's candidates and results).  batch_mb, batch_nb: the last call's sizes (0: none)
	gpemu::DevBuf<double> dBatchW, dBatchLam, dBatchMu, dBatchE, dBatchSv, dBatchDots, dBatchSt, dBatchTab, dBatchIO;
	int batch_mb = 0, batch_nb = 0;
	// gain over a weighted target set (gpemu_design_target_*).  The resident store of tgt_S targets (0: none), S' =
	// tgt_S rounded up to 64: dTgtX their coordinates (S' x d) and dTgtW their weights, both kept across prediction set-ups;
	// dTgtU the u rows (S' x Np), dTgtR the r rows and dTgtQr the [0 | Q r] rows (S' x Rp each), dTgtVar v(x_s), dTgtSum the
	// target variance, all built for the set-up tgt_serial says (pred_serial; 0: to be rebuilt from dTgtX).  Per block of
	// candidates: dTgtCR their r rows, dTgtPanel one panel of U_q U_t^T, dTgtPart its partials, dTgtScr a mean nobody reads, then
	// var and num where the caller keeps neither; dTgtIO the host entries' coordinates and results.  tgt_mb: the candidates of the
	// last block (0: none), whose u and Q r rows are still in dV
	gpemu::DevBuf<double> dTgtX, dTgtW, dTgtU, dTgtR, dTgtQr, dTgtVar, dTgtSum, dTgtCR, dTgtPanel, dTgtPart, dTgtScr, dTgtIO;
	int tgt_S = 0, tgt_mb = 0;
	unsigned long long tgt_serial = 0;
	// calibration against observations (gpemu_calib_*): dCalibTab the resident table of one observation set
	// (kernels_calib.hip has its layout; calib_nt > 0: set up), independent of the model: gpemu_set_model leaves it alone,
	// gpemu_calib_release and the end of the context free it.  dCalibIO / dCalibIdx the host entries' device copies of mean,
	// var and stat / of worst or idx; dCalibCnt the selection's per-workgroup counts, then the total; hCalibCnt that total, pinned
	int calib_nt = 0, calib_nr = 0;
	gpemu::DevBuf<double> dCalibTab, dCalibIO;
	gpemu::DevBuf<int> dCalibIdx, dCalibCnt;
	gpemu::PinnedBuf<int> hCalibCnt;
	gpemu::SampleState sample;   // the ensemble sampler (gpemu_sample_*, gpemu_calib_sample)
	// the input measure of the sensitivity entries per coordinate (gpemu_sens_set_measure): GPEMU_MEASURE_*,
	// all uniform from gpemu_set_model on; kept by gpemu_set_training, the prediction set-ups and gpemu_sens_release
	int sens_kind[GPEMU_MAX_PARAMS] = {};
	gpemu::DevBuf<double> dS;    // corners of (Rp+Np)^2 for explicit inverse / gradient (one per batch element in flight)
	size_t S_dim = 0;            // their side and leading dimension

	// gradient scratch
	gpemu::DevBuf<double> dGradPart;   // tile partial sums of all corners in flight
	// gpemu_symm_apply: a host-resident symmetric matrix kept on the device between calls
	gpemu::DevBuf<double> dSym, dSymV, dSymOut;
	const double *sym_key = nullptr;
	int sym_N = 0, sym_lda = 0, sym_pad = 0;   // sym_pad: padded side and leading dimension of dSym, dSymV, dSymOut
	uint64_t sym_fp = 0;          // checksum of every element of the cached host matrix
	bool sym_pinned = false;      // gpemu_symm_pin: the caller vouches for the buffer, no per-call checksum
	gpemu::DevBuf<gpemu::CovParams> dParams;   // hyper-parameters of the batch elements (GPEMU_MAX_BATCH slots)
	gpemu::DevBuf<double> dAlpha;    // gradient, per corner in flight: Np doubles of alpha = C^-1 y, then GPEMU_MAX_PARAMS length thetas

	int mode = 0;                 // GPEMU_MODE_* flags (gpemu_set_mode; defaults from the environment)
	gpemu::ProfState prof;
	// GPEMU_TRACE=1: per-launch device timestamps (wall_clock64) written by the kernels themselves, so that the
	// concurrent timeline of several contexts can be read (rocprofv3 serialises kernels)
	gpemu::DevBuf<unsigned long long> dTrace;
	int trace_cap = 0, trace_next = 0;
	std::vector<std::string> trace_tag;
	std::vector<double> last_thetas;
private:
	explicit gpemu_ctx() = default;    // made by gpemu_ctx_create and nowhere else (explicit: no aggregate initialisation either)
	friend int gpemu_ctx_create(gpemu_ctx **out, int device);
};

namespace gpemu {

// ---- kernels_cov.hip
hipError_t launch_cov_fill(hipStream_t s, double *out, long ld, const double *Xr, int nr, int nr_pad,
                           const double *Xc, int nc, int nc_pad, int d, const CovParams &p, int mode);
constexpr int FILL_LOWER = 1, FILL_CLAMP = 2, FILL_IDENT_PAD = 4;
// k-vectors of M query rows (padded to Mp) against the design in Gram form (p.gram set; Xg = centred design, mid = its centre)
hipError_t launch_cov_kvec_gram(hipStream_t s, double *out, long ld, const double *Xq, int M, int Mp, const double *X, const double *Xg,
                                const double *mid, int N, int Np, int d, const CovParams &p);
hipError_t launch_build_rrows(hipStream_t s, double *R, int Np, int Rp, const double *X, const double *y,
                              int N, int d, int order);
hipError_t launch_set_identity_rows(hipStream_t s, double *T, long ld, int n, int nbatch = 1, long bstride = 0);
hipError_t launch_cov_stage_batch(hipStream_t s, double *T, long ld, long bstride, int nb, const double *X, int N, int Np, int d,
                                  const CovParams *pp_dev, int mode, const double *Rrows, int Rp, const double *Xg = nullptr,
                                  bool all_gram = false, int kind = GPEMU_POWEREXP, long rstride = 0);
hipError_t launch_transpose(hipStream_t s, double *dst, long ldd, const double *src, long lds, int n);
hipError_t launch_predict_finish(hipStream_t s, const double *V, long ldv, int M, int Np, int nreg, int order, int d,
                                 const double *Xq, const double *betaQ, double kappa, double *mean, double *var,
                                 int nslice = 1, long sstride = 0);
// the few-queries path of the prediction sweep (emulate_point): k-vectors of up to 16 queries, one thread per design point; the
// epilogue with the slice sums fused in, one workgroup per query
hipError_t launch_kvec_small(hipStream_t s, double *Kq, long ld, const double *Xq, int M, const double *X, int N, int Np, int d,
                             const CovParams &p);
hipError_t launch_predict_finish_small(hipStream_t s, const double *Vp, long ldv, long sstride, int nslice, int M, int Np, int nreg,
                                       int d, const double *Xq, const double *betaQ, double kappa, double *mean, double *var);
// the mean-only sweep (gpemu_predict_mean): partial sums k*.gamma per (design slice, query) without storing a k-vector, then
// their sum in slice order plus h^T beta.  part: predict_mean_slices(Np) rows of pstride >= M doubles.
int predict_mean_slices(int Np);
hipError_t launch_predict_mean(hipStream_t s, double *part, long pstride, const double *Xq, int M, const double *X, const double *Xg,
                               const double *mid, const double *gamma, int N, int Np, int d, const CovParams &p, bool gram);
hipError_t launch_predict_mean_finish(hipStream_t s, const double *part, long pstride, int nslice, int M, int nreg, int d,
                                      const double *Xq, const double *beta, double *mean);
// the mean and its gradient with respect to the query point (gpemu_predict_mean_grad): per (design slice,
// query) the mean's partial sum and predict_mean_grad_width(d) sums [S_0, S_1 .. S_d], then the finish in slice order
int predict_mean_grad_width(int d);
hipError_t launch_predict_mean_grad(hipStream_t s, double *mpart, double *gpart, long pstride, const double *Xq, int M, const double *X,
                                    const double *Xc, const double *mid, const double *gamma, int N, int Np, int d, const CovParams &p,
                                    bool gram);
hipError_t launch_predict_mean_grad_finish(hipStream_t s, const double *mpart, const double *gpart, long pstride, int nslice, int M,
                                           int nreg, int d, const double *Xq, const double *mid, const double *beta, const CovParams &p,
                                           double *mean, double *grad);
// the variance's gradient (gpemu_predict_var_grad): (Q r) per query into V's columns Np .. Np + Rp, the fused
// sweep over A^T (Np x lda, the second product's output), the finish in slice order
hipError_t launch_predict_qr(hipStream_t s, double *V, long ldv, int M, int Np, int Rp, int nreg, int d, const double *Xq,
                             const double *betaQ, double *rkeep = nullptr);
// the joint posterior covariance (gpemu_predict_cov): c(x*_p, x*_q) + r_p . (Q r)_q on the lower 64 x 64 tiles of
// S (M x M, leading dimension lds) -- R: the r rows predict_qr kept (M x ldr), V: its Q r in columns Np + 1 .. --, and the copy
// of the strict lower triangle into the upper one
hipError_t launch_predict_cov_prior(hipStream_t s, double *S, long lds, const double *Xq, int M, int d, const CovParams &p,
                                    const double *R, long ldr, const double *V, long ldv, int Np, int nreg);
hipError_t launch_predict_cov_mirror(hipStream_t s, double *S, long lds, int M);
// hold-out validation and joint draws (gpemu_predict_joint_factor / _draw) on the tall matrix T = [S ; 64
// right-hand-side rows], (Mp + 64) x Mp, Mp = M rounded up to 64: noise on the diagonal (var = the diagonal as factored), the
// identity pad and the rows yobs_a - mean in one pass; everything above the diagonal of the factored rows zeroed; the normals
// of nd <= 65535 draws zero-padded to Mp columns and their out rows pre-filled with the mean
hipError_t launch_joint_stage(hipStream_t s, double *T, long ld, int M, const double *noise, const double *mean, const double *yobs,
                              int nobs, double *var);
hipError_t launch_joint_clean(hipStream_t s, double *T, long ld, int Mp);
hipError_t launch_joint_draw_stage(hipStream_t s, double *Zp, long ldz, const double *z, int M, int nd, double *out, const double *mean);
hipError_t launch_transpose_rect(hipStream_t s, double *dst, long ldd, const double *src, long lds, int rows, int cols);
hipError_t launch_predict_var_grad(hipStream_t s, double *gpart, long pstride, const double *Xq, int M, const double *X, const double *Xc,
                                   const double *mid, const double *At, long lda, int N, int Np, int d, const CovParams &p, bool gram);
hipError_t launch_predict_var_grad_finish(hipStream_t s, const double *gpart, long pstride, int nslice, int M, int nreg, int d,
                                          const double *Xq, const double *mid, const double *V, long ldv, int Np, const CovParams &p,
                                          double *grad);
hipError_t launch_grad_partials(hipStream_t s, const double *S, long lds, int soff, long sstride, int nb, const double *X, int N,
                                int d, double *ag, int np_pad, long gstride, double *part, long pstride, int *nparts,
                                int exact_kind = 0, int nbeta = 0, const CovParams *pp_dev = nullptr, bool lit_noclamp = false,
                                const double *Xg = nullptr);

hipError_t launch_beta_solve(hipStream_t s, const double *res, long rstride, int Rp, int nreg, int nb, double *ag, long gstride,
                             int np_pad);
hipError_t launch_grad_reduce(hipStream_t s, const double *part, long pstride, int ntiles, int np, int nb, double *sums, long sstride);

hipError_t launch_deriv_gauss(hipStream_t s, double *out, long ld, const double *xcol, int n, double theta_len);
hipError_t launch_trace_product(hipStream_t s, const double *A, const double *B, long ld, int n, double *part);

// ---- kernels_linalg.hip
hipError_t launch_gemm(hipStream_t s, const GemmArgs &a);
hipError_t launch_skinny_nt(hipStream_t s, const double *Kq, long ldk, const double *L, long ldl, double *Vp, long ldv,
                            long sstride, int tq, int ntot, int K, int ntri, int nslice, int klen);
hipError_t launch_gemv_tri(hipStream_t s, const double *Kq, long ldk, const double *L, long ldl, double *Vp, long ldv,
                           long sstride, int mq, int ntot, int K, int ntri, int nslice, int klen);
std::vector<int> build_tile_table(int tiles_m, int tiles_n, int tri, int S, int bm = 128, int bn = 128);
std::vector<int> build_row_table(int tiles_m, int bm, int kstart_off, int k0, int k1);
hipError_t launch_leaf(hipStream_t s, double *T, long ld, int c0, int m_below, int *info,
                       unsigned long long *trace_factor = nullptr, unsigned long long *trace_solve = nullptr,
                       int nbatch = 1, long bstride = 0, bool skip_factor = false, int staged = -1, bool pre = true, int c0b = -1);
hipError_t launch_leaf_pair(hipStream_t s, double *T, long ld, int c0, int m_below, int *info, unsigned long long *trace, int nbatch,
                            long bstride, bool fa);
// the m_far rows from r_far on under the finished 256-column group at cg, all of the group's arithmetic in one pass
// (panel_rows_kernel).  hipErrorInvalidValue, before anything runs: m_far no positive multiple of 64, r_far < cg + 256, an odd
// ld, bstride or cg, T not 16-byte aligned
hipError_t launch_panel_rows(hipStream_t s, double *T, long ld, int cg, int r_far, int m_far, unsigned long long *trace, int nbatch,
                             long bstride);
bool gemm_factor_ahead_ok(const GemmArgs &a);
bool gemm_uses_big_tiles(const GemmArgs &a);
bool gemm_ride_ok(const GemmArgs &a);
hipError_t launch_gram_partials(hipStream_t s, const double *Z, long ld, int Np, int nrhs, int Rp, double *part,
                                int nbatch = 1, long zstride = 0);
hipError_t launch_finish(hipStream_t s, const double *part, int nparts, int Rp, int nrhs, const double *T, long ld,
                         int N, double *res, int nbatch = 1, long tstride = 0, long rstride = 0);
// leave-one-out (gpemu_loo): column sums of squares of the lower triangle of L^-1 as partials per (row chunk, column), then
// their fixed-order sum with the regression term, mean and variance per training point.  part: loo_scratch_elems doubles.
size_t loo_scratch_elems(int N, int Np);
hipError_t launch_loo_colsq(hipStream_t s, const double *LinvAug, long ld, int N, int Np, double *part);
hipError_t launch_loo_finish(hipStream_t s, const double *part, const double *LinvAug, long ld, int N, int Np, int nreg,
                             const double *betaQ, const double *y, double *mean, double *var);
// leave-group-out (gpemu_lgo) on nbc groups padded to bp, the groups g0 .. g0 + nbc - 1 of a call.  Tables:
// colrow[i] = g * bp + position of design point i in its group g (-1: in none), members = the design indices group after group,
// moff[g] / bsize[g] = where group g starts in members / how many it has.
// gather: column i of L^-1 (rows [0, N) of LinvAug, k >= i only) -> row colrow[i] - g0 * bp of Z (nbc * bp rows of Np), zeros elsewhere
hipError_t launch_lgo_gather(hipStream_t s, const double *LinvAug, long ld, int N, int Np, const int *colrow, const int *bsize,
                             int g0, int nbc, int bp, double *Z);
// staging of the tall matrices T (nbc x (2 bp + 64) x bp, the lower 64 x 64 tiles holding (C^-1)_BB): minus w_i^T Q w_j, identity
// pad, gamma_B as right-hand-side row 0, identity rows
hipError_t launch_lgo_stage(hipStream_t s, double *T, long tstride, int g0, int nbc, int bp, const int *members, const int *moff,
                            const int *bsize, const double *LinvAug, long ld, int Np, int nreg, const double *betaQ);
// finish after the factorisation: var, mean, werr scattered to design order, maha / logdet / logpdf and the decoded info word
// per group.  res: {|w|^2, 2 sum log R_ii} per group of the chunk, info: the chunk's info words
hipError_t launch_lgo_finish(hipStream_t s, const double *T, long tstride, int nbc, int bp, const int *members, const int *moff,
                             const int *bsize, const int *info, const double *res, const double *y, int g0, int ngroups,
                             double *mean, double *var, double *werr, double *stat, int *info_out);

// ---- kernels_sens.hip: closed-form sensitivity analysis of the posterior mean
// prep: sens_prep_elems doubles, table q (I, J^1, J^2, J^3, Pex) of context c at ((c * 5 + q) * d + l) * N + i; cst: SENS_CST_ROWS
// rows of GPEMU_MAX_PARAMS; meas: SensBox::meas of the call, which picks the sweep's instantiation; part: sens_part_elems doubles, 2 d + 1 sums per 64 x 64 tile; out: e0a, e0b, cov_all, first[d], rest[d]
size_t sens_prep_elems(int N, int d);
size_t sens_part_elems(int N, int d);
hipError_t launch_sens_prep(hipStream_t s, const double *X, int N, const SensBox &bx, double *prep, double *cst);
hipError_t launch_sens_sweep(hipStream_t s, const double *X, int N, int d, const double *gamA, const double *gamB, const double *prep,
                             const double *cst, int meas, double *part);
hipError_t launch_sens_finish(hipStream_t s, const double *part, int N, int d, int order, const double *gamA, const double *betaA,
                              double ampA, const double *gamB, const double *betaB, double ampB, const double *prep, const double *cst,
                              double *out);
hipError_t launch_sens_main(hipStream_t s, const double *X, int N, int d, int order, const double *gam, const double *beta, double amp,
                            const double *prep, const double *cst, const double *grid, int ngrid, double *e0, double *out);
// emulator uncertainty.  S: the corner of gpemu_get_cinverse (leading dimension lds, C^-1 at (Rp, Rp), W in
// columns 1 .. nreg); Pw: (N rounded up to 64)^2 doubles, Pw[i' * ldp + i] = P_ii' on the lower tiles; G: N x nreg; part:
// sens_post_part_elems doubles, 2 d + 2 sums per lower tile; out: s_none, s_all, first[d], rest[d]
size_t sens_post_part_elems(int N, int d);
hipError_t launch_sens_pmat(hipStream_t s, const double *S, long lds, int Rp, const double *Q, int N, int nreg, double *G, double *Pw);
hipError_t launch_sens_sweep_weighted(hipStream_t s, const double *X, int N, int d, const double *prep, const double *cst, int meas,
                                      const double *Pw, double *part);
hipError_t launch_sens_post_finish(hipStream_t s, const double *part, int N, int d, int order, int nreg, double amp, const double *prep,
                                   const double *cst, const double *G, const double *Q, double *out);
// the band: rows r0 .. r0 + mb of the d ngrid + 1 into Kq (mbp rows of Np); then the finish over V = Kq LinvAug^T
hipError_t launch_sens_tvec(hipStream_t s, const double *X, int N, int Np, int d, double amp, const double *prep, const double *cst,
                            const double *grid, int ngrid, int r0, int mb, int mbp, double *Kq);
hipError_t launch_sens_band_finish(hipStream_t s, const double *V, long ldv, int mb, int r0, int Np, int nreg, int d, int ngrid,
                                   const double *cst, const double *grid, const double *betaQ, double amp, double *main, double *var);
// second order, npairs = d (d - 1) / 2, pair (j < k) at p = j (2 d - j - 1) / 2 + (k - j - 1).  pex2:
// sens_pex2_elems doubles, Pex2_jk(i) of context c at (c * npairs + p) * N + i, from the I table of prep; part:
// sens_pair_part_elems doubles, npairs sums per 64 x 64 tile (Pw given: per lower tile, weighted, context 0 alone); out: npairs
size_t sens_pex2_elems(int N, int d);
size_t sens_pair_part_elems(int N, int d);
hipError_t launch_sens_pair_prep(hipStream_t s, const double *prep, int N, int d, double *pex2);
hipError_t launch_sens_pair_sweep(hipStream_t s, const double *X, int N, int d, const double *gamA, const double *gamB, const double *pex2,
                                  const double *cst, int meas, const double *Pw, double *part);
hipError_t launch_sens_pair_finish(hipStream_t s, const double *part, int N, int d, int order, const double *gamA, const double *betaA,
                                   double ampA, const double *gamB, const double *betaB, double ampB, const double *prep, const double *cst,
                                   double *out);
hipError_t launch_sens_pair_post_finish(hipStream_t s, const double *part, int N, int d, int nreg, double amp, const double *prep,
                                        const double *cst, const double *G, const double *Q, double *out);
// the two-way surface of the pair j < k at npts points (xj[g], xk[g]): e0, joint[npts], inter[npts]
hipError_t launch_sens_joint(hipStream_t s, const double *X, int N, int d, int order, const double *gam, const double *beta, double amp,
                             const double *prep, const double *pex2, const double *cst, int j, int k, int npts, const double *xj,
                             const double *xk, double *e0, double *joint, double *inter);

// ---- kernels_design.hip: expected IMSE reduction of candidate runs
// KH: design_kh_elems doubles, rows [0, Np) = K (Np x Np, zero from N on), rows Np + al = HK_al; Hm: 64 x 64; prep: the design's
// tables of context 0, prepq: those of the block's mb candidates; Am (mb x lda): the rows of a, Tm (mb x ldt) = a [K | HK];
// part: ceil(N / 64) rows of pstride >= mb partials; V, R: the prediction's [u | . | Q r] rows and the r rows of predict_qr
size_t design_kh_elems(int Np);
hipError_t launch_design_kmat(hipStream_t s, const double *X, int N, int Np, int d, int nreg, const double *prep, const double *cst, int meas,
                              double *KH, double *Hm);
hipError_t launch_design_kvec(hipStream_t s, const double *X, int N, int Np, int d, const double *cst, double amp, const double *Xq, int mb,
                              int mbp, double *Kq);
hipError_t launch_design_cross(hipStream_t s, const double *X, int N, int d, const double *Xq, int mb, const double *cst, int meas,
                               const double *Am, long lda, const double *Tm, long ldt, double *part, long pstride);
hipError_t launch_design_finish(hipStream_t s, const double *part, long pstride, int N, const double *V, long ldv, const double *R, long ldr,
                                const double *Tm, long ldt, const double *prepq, const double *Xq, int mb, int Np, int d, int nreg,
                                const double *cst, int meas, const double *Hm, double amp, double kappa, double *gain, double *num, double *var,
                                double *bkeep);
// greedy batches (gpemu_design_batch).  W: the rows of w (mbp x Np); sv: design_batch_sv_elems doubles, what the
// gather lays out of one pick; Lam, Mu: mb rows of ldl, entry j written by pick j; E: 256 x 256; dots: four rows of dstride;
// vS, numS, gain: the running v_S, num_S and gain of every candidate; pick: the picks so far, in device memory
size_t design_batch_sv_elems(int Np);
hipError_t launch_design_wrows(hipStream_t s, const double *X, int N, int Np, int d, const double *cst, int meas, const double *Xq, int mb,
                               int mbp, double *W);
hipError_t launch_design_gather(hipStream_t s, const int *pick, int j, const double *X, int N, int Np, int d, int nreg, const double *cst,
                                double amp, const double *Xq, int mb, const double *Am, const double *Tm, long ldt, const double *Wm,
                                const double *Bm, const double *prepq, const double *Hm, const double *Lam, const double *Mu, long ldl,
                                const double *vS, const double *numS, double *E, double *sv);
hipError_t launch_design_column(hipStream_t s, const double *Am, const double *Tm, long ldt, const double *Wm, int Np, int mb, const double *sv,
                                double *dots, long dstride);
hipError_t launch_design_update(hipStream_t s, int j, const double *Xq, int mb, int Np, int d, int nreg, const double *cst, int meas, double amp,
                                const double *Tm, long ldt, const double *Bm, const double *prepq, const double *sv, const double *dots,
                                long dstride, double *Lam, double *Mu, long ldl, double *vS, double *numS, double *gain);
hipError_t launch_design_argmax(hipStream_t s, const double *const *gains, const double *weight, int nctx, int M, int *picked, int slot,
                                int *pick, double *pick_gain, double *pick_gain_ctx, double *wout);
// gain over a weighted target set (gpemu_design_target_*).  sweep: mb candidates (Xq; Rq their r rows) against the
// ns targets from s0 on (a multiple of 64) of the S in Xt (QRt: the targets' [0 | Q r] rows, wt their weights); P (mb x ldp) =
// U_q U_t^T of exactly those targets, p: the covariance parameters with nug = 0; part: ceil(ns / 64) rows of pstride >= mb.
// finish: the running num over a panel's ntile partial rows, the quotient behind the last panel.  var: sum_s wt_s vt_s into out[0]
hipError_t launch_design_target_sweep(hipStream_t s, const double *Xq, int mb, const double *Xt, int S, int s0, int ns, int d,
                                      const CovParams &p, const double *P, long ldp, const double *Rq, long ldr, const double *QRt, long ldq,
                                      const double *wt, int nreg, double *part, long pstride);
hipError_t launch_design_target_finish(hipStream_t s, const double *part, long pstride, int ntile, int mb, bool first, bool last,
                                       const double *var, double *num, double *gain);
hipError_t launch_design_target_var(hipStream_t s, const double *wt, const double *vt, int S, double *out);

// ---- kernels_calib.hip: implausibility and calibration likelihood against observations
// the device table of one observation set: calib_table_elems doubles, filled on the host from gpemu_calib_project's outputs
// (sdiag: S_tt per output); eval: mean, var component-major with leading dimension ld, stat 5 x M, worst M; select: counts
// calib_select_blocks(M) + 1 ints (the total kept is left in the last one), idx M ints
int calib_pad(int nr);
size_t calib_table_elems(int nt, int nr);
void calib_fill_table(int nt, int nr, const double *ybar, const double *A, const double *z, const double *sdiag, const double *rel,
                      const double *mhat, const double *sigz, const double *consts, double *tab);
hipError_t launch_calib_eval(hipStream_t s, const double *tab, int nt, int nr, int M, const double *mean, const double *var, long ld,
                             double *stat, int *worst);
// grad: gmean, gvar component-major blocks of M x d with leading dimension ldg; gchi2, glogpdf M x d,
// point-major, either may be null
hipError_t launch_calib_grad(hipStream_t s, const double *tab, int nr, int M, int d, const double *mean, const double *var, long ld,
                             const double *gmean, const double *gvar, long ldg, double *gchi2, double *glogpdf);
int calib_select_blocks(int M);
hipError_t launch_calib_gather(hipStream_t s, const double *stat, const int *worst, int M, int count, const int *idx, double *out, int *wout);
hipError_t launch_calib_select(hipStream_t s, const double *stat, int M, double cut_chi2, int level, double cut_I, int *counts, int *idx);

// ---- kernels_sample.hip: the ensemble sampler's launches
// prior: SAMPLE_PRIOR_ROWS rows of GPEMU_MAX_PARAMS, filled on the host by sample_fill_prior (kind may be null: all uniform);
// x: W x d, y: W / 2 x d, aux: (d - 1) log z of the W / 2 active walkers, then the log prior of their proposals
constexpr int SAMPLE_PRIOR_ROWS = 4;
void sample_fill_prior(int d, const int *kind, const double *lo, const double *hi, double *tab);
hipError_t launch_sample_propose(hipStream_t s, const double *prior, int W, int d, int half, unsigned long long step,
                                 unsigned long long seed, double a, const double *x, double *y, double *aux);
hipError_t launch_sample_accept(hipStream_t s, int W, int d, int half, unsigned long long step, unsigned long long seed, const double *y,
                                const double *aux, const double *loglik, double *x, double *lp, int *nacc);
hipError_t launch_sample_logpost(hipStream_t s, const double *prior, int M, int d, const double *x, const double *loglik, double *lp);

} // namespace gpemu
