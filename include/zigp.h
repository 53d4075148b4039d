/* libzigp -- C-ABI of the MI355X-native zero-inflated ("OnOff") sparse variational GP engine.
 *
 * The reference (hegdepashupati/zero-inflated-gp) is pure Python on TensorFlow 1.x / GPflow 0.4.0 and
 * has NO FFI / plugin / operator interface of its own.  The narrowest seams on
 * its ELBO hot path are Python methods; each entry point below names the reference code it replaces
 * (file:line relative to the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer
 * would add on the reference side.
 *
 * Conventions: every function returns 0 on success and < 0 on error (never throws across the ABI):
 *   ZIGP_EARG  bad argument        ZIGP_EHIP   HIP runtime error        ZIGP_ECOMM  RCCL error (zigp_comm_*)
 *   ZIGP_ENOTPD  Cholesky hit a pivot <= rtol * eps * (variance + jitter), rtol = 8 by default: non-positive, or zero to rounding
 *                (tf.cholesky raises InvalidArgumentError on a non-positive pivot; an exactly singular Kuu rounds either way there;
 *                zigp_set_pivot_rtol(ctx, 0) gives that bare `pivot > 0` test); zigp_last_info() returns the 1-based pivot index
 *                within the failing matrix, zigp_last_error() the message (which names the matrix).
 * All arrays are float64, C-contiguous (row-major), owned by the caller.  Pointers are HOST pointers
 * unless the name says "device".  One ctx per GPU; a ctx is not thread-safe; calls are synchronous
 * (all internal streams are joined before returning).  Reductions are fixed-order: results are
 * bit-stable run to run on the same device, chunk size and shard layout.
 */
#ifndef ZIGP_H
#define ZIGP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ZIGP_OK 0
#define ZIGP_EARG (-1)
#define ZIGP_EHIP (-2)
#define ZIGP_ENOTPD (-3)
#define ZIGP_ECOMM (-4)

typedef struct zigp_ctx zigp_ctx;

/* Largest input dimension D of the dense entry points (zigp_elbo, zigp_predict, zigp_predict_device, zigp_prior_kl, zigp_rbf_K,
 * zigp_set_data, zigp_set_data_device, zigp_select_rows; all three parametrisations).  D <= 8 runs the kernels specialised per
 * dimension; 9 <= D <= ZIGP_MAX_D runs the run-time-D ("wide") kernels.  Narrower: the device fit loops (zigp_fit_steps,
 * zigp_fit_steps_mode) and a Linear mean function (zigp_set_mean_function with D > 0) stay at D <= 8, and the Kronecker path has its
 * own fixed factor dimensions.  A larger D is ZIGP_EARG. */
#define ZIGP_MAX_D 64

/* Constrained parameter values of the dense model.  Replaces the Param members created in
 * OnOffSVGP.__init__ (onoffgpf/OnOffSVGP.py:50-71), the two gpflow.kernels.RBF objects
 * (zero-inflated-gpflow.ipynb:98-104; twin KernSE onofftf/main.py:33-63) and
 * OnOffLikelihood.variance (onoffgpf/OnOffLikelihood.py:26).
 * 1 <= D <= ZIGP_MAX_D (64).  ell_*: D lengthscales (ARD; broadcast a scalar on the host). u_*s_sqrt: diagonal q_sqrt (q_diag=True,
 * OnOffSVGP.py:34). */
typedef struct {
  int32_t Mf, Mg, D, reserved;
  const double *Zf, *Zg;             /* (Mf,D), (Mg,D) inducing inputs */
  const double *u_fm, *u_gm;         /* (Mf), (Mg) variational means */
  const double *u_fs_sqrt, *u_gs_sqrt; /* (Mf), (Mg) variational std-devs (> 0); with zigp_set_q_full: (Mf,Mf), (Mg,Mg) lower-triangular factors */
  const double *ell_f, *ell_g;       /* (D), (D) */
  double var_f, var_g;               /* kernel variances */
  double noise;                      /* likelihood variance */
} zigp_params;

/* Gradient of the returned ELBO w.r.t. the constrained values above (same shapes). The host applies
 * the Log1pe ("positive" transform) chain rule, as GPflow's Param / onofftf Param.get_tfv do
 * (onofftf/main.py:170-174). */
typedef struct {
  double *Zf, *Zg, *u_fm, *u_gm, *u_fs_sqrt, *u_gs_sqrt, *ell_f, *ell_g;
  double var_f, var_g, noise;
} zigp_grads;

int zigp_create(zigp_ctx** out, int device_id);
int zigp_destroy(zigp_ctx* ctx);
const char* zigp_last_error(zigp_ctx* ctx);
int zigp_last_info(zigp_ctx* ctx);

/* Tunables: chunk = number of data rows processed per pass through the fused pipeline (multiple of
 * 1024 and <= 1048576).  Default, until this is called: 32768 * 1024 / M rows, clamped to [32768, 131072]; a row range of up to 131072
 * rows goes through in one pass while 4 panels of 8 * M * rows bytes per latent stay within 9 GB (a pass holds 3: K, A1 and J'; the
 * bound is deliberately conservative).  chunk_rows = 0 returns to that default rule. */
int zigp_set_chunk(zigp_ctx* ctx, int64_t chunk_rows);
/* The chunk (rows per pass) the dense path uses for M inducing points per latent on a long row range: the zigp_set_chunk value, else
 * the default rule. */
int64_t zigp_get_chunk(zigp_ctx* ctx, int32_t M);
/* Rows per pass the dense path actually uses for a row range of `span` rows: the range is cut into equal passes of at most the chunk above
 * (a multiple of 1024 rows each), and a range of up to 131072 rows goes through in ONE pass while 4 panels of 8 * M * rows bytes per latent
 * (3 held: K, A1, J') stay within 9 GB (M <= 1024). */
int64_t zigp_get_chunk_rows(zigp_ctx* ctx, int32_t M, int64_t span);
/* Smallest Cholesky pivot accepted, as a multiple of eps * (kernel variance + jitter).  Default 8 (see ZIGP_ENOTPD above);
 * 0 reproduces tf.cholesky / LAPACK potrf, which fail on a non-positive pivot only (onofftf/main.py:200,268,355). */
int zigp_set_pivot_rtol(zigp_ctx* ctx, double rtol);

/* Training data.  Replaces the MinibatchData / DataHolder objects of OnOffSVGP.__init__
 * (onoffgpf/OnOffSVGP.py:38-47) and the X/Y feed_dict of scripts/onoff.py:379-381.
 * zigp_set_data copies host arrays into HBM once; zigp_set_data_device adopts device pointers
 * (e.g. torch tensors) without copying -- the caller keeps them alive. X is (N,D), Y is (N). */
int zigp_set_data(zigp_ctx* ctx, const double* X, const double* Y, int64_t N, int32_t D);
int zigp_set_data_device(zigp_ctx* ctx, const double* dX, const double* dY, int64_t N, int32_t D);
/* Minibatch by row indices: the n rows `rows` of the resident set (repeats allowed) are gathered on the device and become the active
 * data, rows [0, n), of the calls that follow -- replaces the per-step sample of GPflow's MinibatchData (onoffgpf/OnOffSVGP.py:46-47)
 * without re-uploading X and Y (8 bytes per row cross the bus instead of 8 (D + 1)).  n = 0: back to the whole resident set;
 * zigp_set_data / zigp_set_data_device reset it. */
int zigp_select_rows(zigp_ctx* ctx, const int64_t* rows, int64_t n);

/* One ELBO evaluation ("step" when grads != NULL) over rows [row_begin, row_end) of the resident data.
 * Replaces OnOffSVGP.build_likelihood (onoffgpf/OnOffSVGP.py:107-122) + its gradient (GPflow
 * Model.optimize -> tf.gradients) i.e. one L-BFGS-B function evaluation / one sess.run(train_op)
 * (scripts/onoff.py:379).
 *   *elbo_data = scale * sum_n var_exp_n  (the data term incl. minibatch scale, OnOffSVGP.py:119-122)
 *   *kl        = KL_f + KL_g              (build_prior_KL, OnOffSVGP.py:96-101); 0 if include_kl == 0
 *   ELBO = *elbo_data - *kl ; grads (nullable) = d ELBO / d params, with the KL part only if include_kl.
 * jitter is added to diag(Kuu) (settings.numerics.jitter_level, OnOffSVGP.py:96-97);
 * g_offset is added to gmean before the probit moments (0 for fit; -1 reproduces onofftf/onoffpred.py:141).
 * Data-parallel use: every rank calls this on its own row shard with include_kl = (rank == 0) and the
 * host sums {elbo_data, kl, grads} over ranks (one all-reduce). */
int zigp_elbo(zigp_ctx* ctx, const zigp_params* p, double jitter, double scale, double g_offset,
              int64_t row_begin, int64_t row_end, int32_t include_kl,
              double* elbo_data, double* kl, zigp_grads* grads);

/* ---- the dense fit loop on the device ---------------------------------------------------------------------------------------------
 * Replaces the body of the dense model's minibatch training loop -- one sample of MinibatchData (onoffgpf/OnOffSVGP.py:42-47), one
 * build_likelihood + gradient (:107-122, scaled by num_data / minibatch_size, :119-120) and one Adam update (the alternative to L-BFGS-B at
 * zero-inflated-gpflow.ipynb:155) -- for n_steps consecutive iterations: gradient of cost = -(scale * sum var_exp - KL), chained through
 * the Log1pe transform of the positive parameters (GPflow transforms.positive: OnOffSVGP.py:61,63, OnOffLikelihood.py:26), Adam with
 * lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), m / (sqrt(v) + eps).  As in zigp_kron_fit_steps the parameters live on the device for the
 * whole call: every step's kernels read the parameter image and the hyperparameter block the previous step's update wrote, the steps are
 * enqueued back to back and the host synchronises ONCE, at the end of the call.
 *   shape        the model's sizes (Mf, Mg, D); its pointer and value fields are ignored
 *   free_state   in/out [n_free]: the UNCONSTRAINED parameters in this block order (ZIGP_DENSE_FIT_BLOCKS = 11, the order of zigp_params):
 *                Zf (Mf x D), Zg (Mg x D), u_fm (Mf), u_gm (Mg), u_fs_sqrt (Mf), u_gs_sqrt (Mg), ell_f, ell_g (ell_size_* entries each),
 *                var_f, var_g, noise
 *   adam_m, adam_v   in/out [n_free]: Adam moments (zeros at iteration 0)
 *   t0           iterations done before this call (step i of the call is Adam's t = t0 + i + 1)
 *   rows         [n_steps * batch] indices into the RESIDENT data set (zigp_set_data), repeats allowed, as for zigp_select_rows: step i
 *                uses rows[i batch .. (i + 1) batch).  They are uploaded once per call and every step gathers its rows on the device into a
 *                buffer of the call's own: the active selection of zigp_select_rows is left as found.  NULL: every step uses the ACTIVE
 *                rows [0, N) (full-batch Adam; `batch` is ignored)
 *   elbo_data, kl    out [n_steps] (nullable): scale * sum var_exp and KL of every step, evaluated at the parameters BEFORE its update
 * opts: per block the learning rate, positive (1: value = log(1 + exp(x)) + 1e-6, Log1pe with lower 1e-6; 0: value = x) and trainable
 * (0: the block's x, m and v stay untouched -- a fixed parameter, which zigp.optim.AdamGroups skips too; its value is the transform of
 * its free-state entry).  ell_size_f / ell_size_g: D, or 1 for ONE lengthscale broadcast over the D columns, whose gradient is the sum
 * of the D per-column gradients in column order.
 * Every step runs the per-row form of the Kuf-cotangent reductions (the centred form of zigp_elbo needs a centre chosen on the host).
 * A Cholesky failure in step k returns ZIGP_ENOTPD; free_state / adam_* then hold the state before the failing step -- the k updates
 * before it HAVE been applied (zigp_fit_steps_applied returns k) -- the history entries from step k on are NaN, and zigp_last_error names
 * the step and the latent.  The steps enqueued behind a failed one still run (at most n_steps - k wasted steps); their updates are skipped.
 * ZIGP_EARG: NULL arguments or bad sizes, n_free not the model's, a row index out of range, more than 1 GiB of row indices, a mean
 * function set on the context (its parameters stay with zigp_elbo and a host optimiser), whitening or the full-covariance q(u) switched on (zigp_set_whiten, zigp_set_q_full) or a
 * communicator attached (zigp_comm_init). */
#define ZIGP_DENSE_FIT_BLOCKS 11
typedef struct {
  double lr[ZIGP_DENSE_FIT_BLOCKS];          /* Adam learning rate of each block */
  int32_t positive[ZIGP_DENSE_FIT_BLOCKS];   /* 1: Log1pe (lower 1e-6), 0: identity */
  int32_t trainable[ZIGP_DENSE_FIT_BLOCKS];  /* 0: fixed */
  int32_t ell_size_f, ell_size_g;            /* 1 or D */
  double beta1, beta2, eps;                  /* TensorFlow's defaults: 0.9, 0.999, 1e-8 */
} zigp_fit_opts;
int zigp_fit_steps(zigp_ctx* ctx, const zigp_params* shape, const zigp_fit_opts* opts, double* free_state, double* adam_m,
                   double* adam_v, int64_t n_free, int64_t t0, int32_t n_steps, const int64_t* rows, int64_t batch,
                   double jitter, double scale, int32_t include_kl, double* elbo_data, double* kl);
/* The same loop for the whitened parametrisations.  `mode` is an argument of the CALL: it decides the model that is fitted and the layout
 * of free_state; the context's zigp_set_whiten / zigp_set_q_full settings are neither read nor changed, and the calls that follow
 * (zigp_elbo, zigp_predict, ...) behave as if this call had not happened.
 *   ZIGP_FIT_DIAG        unwhitened, diagonal q(u): the code path of zigp_fit_steps, bit-identical state and history
 *   ZIGP_FIT_WHITE       zigp_set_whiten's model, q(u) = N(L u, L diag(s^2) L^T); the 11 blocks of zigp_fit_steps
 *   ZIGP_FIT_WHITE_FULL  zigp_set_q_full's model, q(u) = N(L u, L Lq Lq^T L^T).  Blocks 4 and 5 hold the M (M + 1) / 2 entries of the LOWER
 *                        TRIANGLE of Lq in row-major order (entry (i, j), j <= i, at i (i + 1) / 2 + j: the free vector of
 *                        zigp.transforms.LowerTriangular and of GPflow's transforms.LowerTriangular); the diagonal is unconstrained
 *                        (a negative entry is legal), so positive[4] and positive[5] must be 0.  n_free follows from these sizes.
 * Everything else is zigp_fit_steps, word for word: rows / batch / NULL rows, t0, the history taken before each update, one
 * synchronisation per call, and the Cholesky-failure contract (ZIGP_ENOTPD, the state before the failing step, NaN history from step k on,
 * k in zigp_fit_steps_applied -- the two calls share that counter).
 * ZIGP_EARG (nothing enqueued, the state untouched): what zigp_fit_steps refuses except the context's whiten / q_full flags -- a mean
 * function and a communicator included -- and an unknown mode, positive set on a full block, a diagonal entry of Lq that is exactly zero
 * in the incoming free_state (its log is not finite).  A diagonal entry that an update lands on exactly zero gets no special handling:
 * that step's KL is not finite and its history entry shows it (an applied step may have a non-finite ELBO). */
#define ZIGP_FIT_DIAG 0
#define ZIGP_FIT_WHITE 1
#define ZIGP_FIT_WHITE_FULL 2
int zigp_fit_steps_mode(zigp_ctx* ctx, int32_t mode, const zigp_params* shape, const zigp_fit_opts* opts, double* free_state,
                        double* adam_m, double* adam_v, int64_t n_free, int64_t t0, int32_t n_steps, const int64_t* rows,
                        int64_t batch, double jitter, double scale, int32_t include_kl, double* elbo_data, double* kl);
/* Updates applied by the LAST zigp_fit_steps or zigp_fit_steps_mode call of this context: n_steps after a call that returned 0, the k steps
 * before the failing one after ZIGP_ENOTPD, 0 when the call ended before its first step (bad argument, HIP error). */
int64_t zigp_fit_steps_applied(zigp_ctx* ctx);

/* Prediction.  Replaces OnOffSVGP.predict_onoffgp -> build_predict (onoffgpf/OnOffSVGP.py:124-152,160-162).
 * out9 is (9,N): gfmean, gfvar, gfmeanu, fmean, fvar, gmean, gvar, ephi_g, evar_phi_g (order of :152). */
int zigp_predict(zigp_ctx* ctx, const zigp_params* p, const double* Xnew, int64_t N, double jitter,
                 double g_offset, double* out9);
/* The same with Xnew (N,D) and out9 (9,N) in DEVICE memory of the context's GPU (the companion of zigp_set_data_device): nothing crosses
 * PCIe but the parameters; complete on return.  The caller orders its own streams around the call (it is synchronous on the host). */
int zigp_predict_device(zigp_ctx* ctx, const zigp_params* p, const double* dXnew, int64_t N, double jitter,
                        double g_offset, double* d_out9);

/* Prior KL only (OnOffSVGP.compute_prior_KL, onoffgpf/OnOffSVGP.py:164-166): kl2 = {KL_f, KL_g}. */
int zigp_prior_kl(zigp_ctx* ctx, const zigp_params* p, double jitter, double* kl2);

/* RBF kernel matrices (gpflow.kernels.RBF.K / KernSE.K onofftf/main.py:53-57; kernse_np.K
 * onofftf/utils.py:48-52): K (n1,n2) = var * exp(-0.5 * sum_d ((x1-x2)/ell_d)^2).  X2 == NULL -> X1. */
int zigp_rbf_K(zigp_ctx* ctx, const double* X1, int64_t n1, const double* X2, int64_t n2, int32_t D,
               const double* ell, double var, double* K);

/* ---- Kronecker (space x time) variant: scripts/onoff.py:143-319, onofftf/main.py:350-387 ---- */
/* Two factors (the reference's Khatri-Rao line scripts/onoff.py:206 is written for exactly two):
 * factor 0 acts on the first D0 input columns, factor 1 on the next D1 (scripts/onoff.py:243-250).
 * u_* and u_*s_sqrt have M0*M1 entries, factor-0-major (row = i*M1 + j, scripts/onoff.py:206). */
typedef struct {
  int32_t M0f, M1f, M0g, M1g, D0, D1, reserved0, reserved1;
  const double *Z0f, *Z1f, *Z0g, *Z1g;       /* (M0,D0), (M1,D1) */
  const double *ell0f, *ell1f, *ell0g, *ell1g; /* (D0), (D1) */
  double var0f, var1f, var0g, var1g;
  const double *u_fm, *u_gm, *u_fs_sqrt, *u_gs_sqrt;
  double noise;
} zigp_kron_params;

typedef struct {
  double *Z0f, *Z1f, *Z0g, *Z1g, *ell0f, *ell1f, *ell0g, *ell1g;
  double var0f, var1f, var0g, var1g;
  double *u_fm, *u_gm, *u_fs_sqrt, *u_gs_sqrt;
  double noise;
} zigp_kron_grads;

/* ELBO / step on an explicit minibatch (host arrays), as scripts/onoff.py:377-381 feeds it.
 * Replaces build_prior_kl + build_predict/kron_inf + cost (scripts/onoff.py:143-213,286-319). */
/* f_mu: the optional constant added to fmean (`if not f_mu is None: fmean = fmean + f_mu.get_tfv()`, scripts/onoff.py:161,168-169;
 * onofftf/onoffpred.py:127,135-136; pass 0 for the reference's default f_mu=None); d_f_mu (nullable) receives its gradient. */
int zigp_kron_elbo(zigp_ctx* ctx, const zigp_kron_params* p, const double* X, const double* Y, int64_t N,
                   double jitter, double scale, double g_offset, double f_mu, int32_t include_kl,
                   double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu);
/* The same step on rows [row_begin, row_end) of the RESIDENT data set (zigp_set_data / zigp_set_data_device, D = D0 + D1): no
 * host->device copy of the minibatch.  The reference's iterator (DataSet.next_batch, onofftf/main.py:98-133) shuffles once per
 * epoch and then hands out contiguous slices, so a host that makes the permuted epoch resident feeds every step by row range;
 * the full-batch configuration (BASELINE cfg5) is rows [0, N). */
int zigp_kron_elbo_rows(zigp_ctx* ctx, const zigp_kron_params* p, int64_t row_begin, int64_t row_end, double jitter, double scale,
                        double g_offset, double f_mu, int32_t include_kl, double* elbo_data, double* kl, zigp_kron_grads* grads,
                        double* d_f_mu);
/* Replaces predict_onoff's graph (onofftf/onoffpred.py:127-200); out9 as zigp_predict. */
int zigp_kron_predict(zigp_ctx* ctx, const zigp_kron_params* p, const double* Xnew, int64_t N, double jitter,
                      double g_offset, double f_mu, double* out9);

/* ---- the fit loop on the device --------------------------------------------------------------------------------------------------
 * Replaces the reference's training loop body, scripts/onoff.py:375-381 (`sess.run(train_op)` on `train_data.next_batch(num_minibatch)`),
 * for n_steps consecutive iterations: gradient of cost = -(scale * sum var_exp - KL) (:318,334), chained through the Log1pe transform of
 * the positive parameters (GPflow transforms.positive, :88-123), one tf.train.AdamOptimizer per learning rate (:325-350; lr_t =
 * lr sqrt(1 - beta2^t) / (1 - beta1^t), m / (sqrt(v) + eps)).  The parameters live on the device for the whole call: every step's
 * kernels read the parameter image the previous step's update wrote, the steps are enqueued back to back on one stream and the host
 * synchronises ONCE, at the end of the call (the reference logs every 200 iterations, :418: call it with n_steps = 200).
 *   shape        the model's sizes (M0f .. D1); its pointer and value fields are ignored
 *   free_state   in/out [n_free]: the UNCONSTRAINED parameters in this block order -- for latent f, then g: Z0 (M0 x D0), Z1 (M1 x D1),
 *                u_m (M0 M1), u_s_sqrt (M0 M1), ell0 (D0), ell1 (D1), var0, var1; then the likelihood variance (ZIGP_FIT_BLOCKS = 17 blocks)
 *   adam_m, adam_v   in/out [n_free]: Adam moments (zeros at iteration 0)
 *   t0           iterations done before this call (the first step of the call is Adam's t = t0 + 1)
 *   row_begin    [n_steps]: step i uses rows [row_begin[i], row_begin[i] + batch) of the RESIDENT data set (zigp_set_data; the permuted
 *                epoch, onofftf/main.py:98-133); a negative value -(1 + k) selects rows [k batch, (k + 1) batch) of the host arrays Xw, Yw
 *                instead (the one wrap-around batch per epoch, which is a concatenation of the old and the new permutation, :125-129)
 *   elbo_data, kl    out [n_steps] (nullable): scale * sum var_exp and KL of every step, evaluated at the parameters BEFORE its update
 * Grids beyond the fused kernels (a factor of more than 32 points next to one of more than 16, or more than 112) return ZIGP_EARG: step
 * them with zigp_kron_elbo_rows and a host optimiser.  A Cholesky failure in step k returns ZIGP_ENOTPD; free_state / adam_* then hold the state
 * before the failing step -- the k updates before it HAVE been applied: the caller's iteration count advances by k -- and the history
 * entries from step k on are NaN (the finite prefix is the history of the applied steps).  With a communicator (zigp_comm_init) every step's result
 * block is summed over the ranks before its update, so all ranks hold the same parameters (each passes its own rows, include_kl as usual
 * is rank 0's). */
#define ZIGP_FIT_BLOCKS 17
typedef struct {
  double lr[ZIGP_FIT_BLOCKS];          /* Adam learning rate of each block */
  int32_t positive[ZIGP_FIT_BLOCKS];   /* 1: value = log(1 + exp(x)) + 1e-6 (Log1pe), 0: value = x */
  int32_t reserved;
  double beta1, beta2, eps;            /* TensorFlow's defaults: 0.9, 0.999, 1e-8 */
} zigp_kron_fit_opts;
int zigp_kron_fit_steps(zigp_ctx* ctx, const zigp_kron_params* shape, const zigp_kron_fit_opts* opts,
                        double* free_state, double* adam_m, double* adam_v, int64_t n_free,
                        int64_t t0, int32_t n_steps, const int64_t* row_begin, int64_t batch,
                        const double* Xw, const double* Yw, double jitter, double scale, int32_t include_kl,
                        double* elbo_data, double* kl);
/* Updates applied by the LAST zigp_kron_fit_steps or zigp_kron_head_fit_steps call of this context (one counter for both): n_steps after a call that returned 0, the k steps before the failing
 * one after ZIGP_ENOTPD, 0 when the call ended before its first step (bad argument, HIP error).  This -- not a scan of the history for
 * NaN: an applied step may itself have a non-finite ELBO -- is what the caller's iteration count and Adam's bias correction advance by. */
int64_t zigp_kron_fit_steps_applied(zigp_ctx* ctx);

/* Mean function of the latent f: m(x) = b + a . x, added to fmean before the likelihood and in zigp_predict
 * (`fmean = fmean + self.mean_function(Xnew)`, onoffgpf/OnOffSVGP.py:29,134).  Covers GPflow's Zero (the reference default:
 * D = -1 -- the state after zigp_create; a and b are ignored), Constant (D = 0, b = c; enabled also when c == 0, so that the
 * parameter still receives its gradient) and Linear with one output (a[D], b; D <= 8 -- Zero and Constant work at every input dimension,
 * a Linear mean at more than 8 columns is ZIGP_EARG).  The setting
 * persists in the context.  zigp_get_mean_function_grad returns d(scale * sum var_exp)/d(a, b) of the LAST zigp_elbo
 * called with grads != NULL (zeros when the mean function is off); like the other gradients it is a per-shard partial
 * sum under data-parallel use. */
int zigp_set_mean_function(zigp_ctx* ctx, const double* a, int32_t D, double b);
int zigp_get_mean_function_grad(zigp_ctx* ctx, double* da, int32_t D, double* db);

/* Whitened variational parametrisation of the DENSE path (the reference's `whiten` switch: gauss_kl_white_diag in build_prior_KL,
 * onoffgpf/OnOffSVGP.py:88-91; whiten=self.whiten into the conditional, :133,137; GPConditional(whiten=True) skips the second
 * back-substitution, onofftf/main.py:282-284; GaussKL(q_mu, q_sqrt, K=None), :193-195,227-228,246).  With on = 1, u_*m and u_*s_sqrt in
 * zigp_params, and the matching blocks of zigp_grads, are the whitened quantities: q(u) = N(L u_m, L diag(u_s_sqrt^2) L^T) with
 * L = chol(Kuu + jitter I), so that
 *   mean = A^T u_m (+ mean function for f),  var = k** + sum_m (u_s_sqrt_m^2 - 1) A_mn^2,  A = L^-1 Kuf,
 *   KL   = 0.5 (sum u_m^2 + sum u_s_sqrt^2 - M - sum log u_s_sqrt^2)   per latent.
 * zigp_elbo (value-only, gradient, include_kl 0 / 1, row ranges, zigp_select_rows), zigp_predict, zigp_predict_device and zigp_prior_kl
 * follow the setting; mean functions, g_offset, scale, the chunk rule and the data-parallel exchange work as without it.  The setting
 * persists in the context like zigp_set_mean_function and is off after zigp_create.  zigp_fit_steps returns ZIGP_EARG while it is on (that
 * call fits the unwhitened parametrisation only; the device loop of this model is zigp_fit_steps_mode with ZIGP_FIT_WHITE, which takes
 * the parametrisation as an argument and does not read this setting); the Kronecker entry points ignore it (the reference raises NotImplementedError
 * there, scripts/onoff.py:145-146).  zigp_get_whiten returns 0 / 1, or ZIGP_EARG for a NULL context. */
int zigp_set_whiten(zigp_ctx* ctx, int32_t on);
int zigp_get_whiten(zigp_ctx* ctx);

/* Full-covariance q(u) of the whitened DENSE model (the reference's `q_diag = False` switch, onoffgpf/OnOffSVGP.py:33-34: the
 * (M, M, num_latent) q_sqrt with transforms.LowerTriangular, :59-71; gauss_kl_white in build_prior_KL, :88-104; the 3-d q_sqrt branches
 * of GaussKL and GPConditional, onofftf/main.py:208-213 and :292-296).  With on = 1 -- and zigp_set_whiten on -- u_fs_sqrt / u_gs_sqrt
 * in zigp_params point to (M, M) row-major arrays of which only the lower triangle Lq is read (band_part(q_sqrt, -1, 0), main.py:210,293:
 * whatever lies above the diagonal is ignored), and q(u) = N(L u_m, L Lq Lq^T L^T) with L = chol(Kuu + jitter I), so that
 *   mean = A^T u_m (+ mean function for f),  var = k** - sum_m A_mn^2 + sum_m (Lq^T A)_mn^2,  A = L^-1 Kuf   (main.py:278,287,293-296,302)
 *   KL   = 0.5 (sum u_m^2 + sum_{i>=j} Lq_ij^2 - M - sum_i log Lq_ii^2)                                  (main.py:193-195,212-213,224,227-228,246).
 * A negative diagonal entry is legal (the log of its square); a zero one is ZIGP_EARG.  The blocks of the same name in zigp_grads are
 * (M, M) with an exactly zero strict upper triangle; the struct layouts do not change.  zigp_elbo (all its options), zigp_predict,
 * zigp_predict_device and zigp_prior_kl follow the setting.  The call's result vector grows to 16 + sum_h (M D + M + M^2 + D) doubles
 * and the parameter upload by M^2 per latent (8 MB each way and latent at M = 1024, through the page-locked arena).
 * ZIGP_EARG, with nothing enqueued: any of those calls while this is on and whitening is off (the unwhitened full-covariance model,
 * gauss_kl, OnOffSVGP.py:102-104, is not implemented), and zigp_fit_steps while it is on (the device loop of
 * this model is zigp_fit_steps_mode with ZIGP_FIT_WHITE_FULL, which does not read this setting).  The setting persists in the context, is off
 * after zigp_create, and the Kronecker entry points ignore it.  zigp_get_q_full returns 0 / 1, or ZIGP_EARG for a NULL context. */
int zigp_set_q_full(zigp_ctx* ctx, int32_t on);
int zigp_get_q_full(zigp_ctx* ctx);

/* Kernel family of the DENSE path, per latent.  Replaces the choice of kernel object handed to the model: "gpflow objects for function &
 * gamma kernels" (onoffgpf/OnOffSVGP.py:22; gpflow.kernels.RBF at zero-inflated-gpflow.ipynb:98-104, for which GPflow 0.4.0's
 * kernels.Matern32 / kernels.Matern52 are drop-in alternatives, each latent its own).  With r2 = sum_d ((x_d - z_d) / ell_d)^2 and
 * r = sqrt(r2 + 1e-12) (Stationary.euclid_dist; the floor keeps coincident points differentiable):
 *   ZIGP_KERN_RBF       k = var exp(-r2 / 2)                               (the state after zigp_create)
 *   ZIGP_KERN_MATERN32  k = var (1 + sqrt3 r) exp(-sqrt3 r)
 *   ZIGP_KERN_MATERN52  k = var (1 + sqrt5 r + (5/3) r^2) exp(-sqrt5 r)
 * Kdiag is var for all three; the diagonal of K(Z, Z) is the formula at r = 1e-6 (plus jitter), as GPflow evaluates it.  latent: 0 = f,
 * 1 = g; the two may differ.  zigp_elbo (value-only and gradient, include_kl 0 / 1, row ranges, zigp_select_rows), zigp_predict,
 * zigp_predict_device and zigp_prior_kl follow the setting in all three parametrisations (zigp_set_whiten, zigp_set_q_full); mean
 * functions, g_offset, scale, the chunk rule and the data-parallel exchange work as without it; zigp_params and zigp_grads keep their
 * layouts (ell_*, var_* are the kernel's lengthscales and variance).  A gradient step keeps one more panel of 8 * M * rows bytes per
 * Matern latent (the derivative factor K' = -dk / d(r2 / 2)), the fourth of the four the chunk rule budgets (zigp_set_chunk).  The
 * setting persists in the context like zigp_set_whiten.
 * ZIGP_EARG: a NULL context, a latent outside {0, 1}, an unknown kind.  While a latent is Matern these return ZIGP_EARG with nothing
 * enqueued (the message names the kernel): the entry points above at D > 8 (the wide kernels are RBF only), and zigp_fit_steps /
 * zigp_fit_steps_mode at every D (the device loops fit RBF latents; zigp_elbo + a host optimiser fits the others).  The Kronecker entry
 * points ignore the setting (theirs is zigp_set_kron_kernel, below).  zigp_get_kernel returns the kind, or ZIGP_EARG for a NULL context or a latent outside {0, 1}. */
#define ZIGP_KERN_RBF 0
#define ZIGP_KERN_MATERN32 1
#define ZIGP_KERN_MATERN52 2
int zigp_set_kernel(zigp_ctx* ctx, int32_t latent /* 0 f, 1 g */, int32_t kind);
int zigp_get_kernel(zigp_ctx* ctx, int32_t latent);
/* Kernel family of the KRONECKER path and its heads, per latent AND per factor: four independent settings (latent f / g x factor 0 / 1),
 * all ZIGP_KERN_RBF after zigp_create, separate from zigp_set_kernel (which keeps meaning the dense latents only).  Per factor q, with
 * r2 formed by fused multiply-adds from 0 in ascending d of (z_d / ell_d - x_d / ell_d) as the RBF factor panel forms it, k_q is the
 * formula block above: r = sqrt(r2 + 1e-12); the diagonal of K_q(Z, Z) is the formula at r = 1e-6, plus jitter; Knn = var0 var1 for every
 * kind.  zigp_kron_elbo[_rows] (value and gradient, include_kl 0 / 1, f_mu, g_offset, an empty row set, a communicator),
 * zigp_kron_predict, zigp_kron_head_elbo[_rows] and zigp_kron_head_predict (the heads read the f kinds), and the sample paths of
 * zigp_kronpaths.h follow the setting.  A call with any Matern factor runs on the GEMM-panel path whatever its grid (the fused
 * register-resident kernels are RBF only; zigp_set_kron_panels is not needed); with all four factors RBF every call launches what it
 * launched before this setting existed.  A gradient step keeps one more panel of 8 * M_q * rows bytes per Matern factor (K').
 * ZIGP_EARG, naming the argument: a NULL context, a latent or factor outside {0, 1}, an unknown kind.  While a factor of a latent they fit
 * is Matern, zigp_kron_fit_steps and zigp_kron_head_fit_steps return ZIGP_EARG with nothing enqueued and the context usable; the message
 * names the kernel, the factor and the latent ("... Matern52 kernel on factor 1 of latent f ...").  Factor dimensions stay D0, D1 <= 8.
 * zigp_get_kron_kernel returns the kind, or ZIGP_EARG. */
int zigp_set_kron_kernel(zigp_ctx* ctx, int32_t latent /* 0 f, 1 g */, int32_t factor /* 0, 1 */, int32_t kind /* ZIGP_KERN_* */);
int zigp_get_kron_kernel(zigp_ctx* ctx, int32_t latent, int32_t factor);
/* Matern factors on the FUSED Kronecker kernels: opt-in context state, 0 after zigp_create.  With it off nothing changes: a call with a
 * Matern factor runs on the GEMM panels, and the fit loops refuse it, as described above.  With it on, a call with a Matern factor goes to
 * the fused register-resident kernels when zigp_set_kron_panels is off and its grid is one they cover (<= 32 x <= 32 or <= 16 x <= 112
 * points, D0, D1 <= 7) -- the Matern instantiations of those kernels, launched only for such a call -- and zigp_kron_fit_steps /
 * zigp_kron_head_fit_steps accept Matern factors (the kinds are fixed for the call).  Every other case routes as with the switch off:
 * zigp_set_kron_panels(1) still wins, a grid beyond the fused kernels stays on the panels, and a call whose four factors are RBF launches
 * what it always launched and returns the same bits.  ZIGP_EARG, naming the argument: a NULL context, on outside {0, 1}.
 * zigp_get_kron_matern_fused returns the setting, or ZIGP_EARG for a NULL context. */
int zigp_set_kron_matern_fused(zigp_ctx* ctx, int32_t on);
int zigp_get_kron_matern_fused(zigp_ctx* ctx);
/* Kernel matrices of any of the three kinds (gpflow kernels.Stationary.K -> RBF.K / Matern32.K / Matern52.K; zigp_rbf_K is the RBF
 * one and stays as it is): K (n1,n2) = k(X1, X2) as above, no jitter.  X2 == NULL -> X1 (the diagonal is then the formula at r = 1e-6
 * for the Matern kinds).  Argument conventions of zigp_rbf_K; 1 <= D <= ZIGP_MAX_D for ZIGP_KERN_RBF, D <= 8 for the Matern kinds. */
int zigp_kern_K(zigp_ctx* ctx, int32_t kind, const double* X1, int64_t n1, const double* X2, int64_t n2, int32_t D,
                const double* ell, double var, double* K);

/* Single-latent heads on the same Kronecker conditional -- the reference's baselines, which re-use kron_inf and
 * GaussKLkron with one latent f:
 *   ZIGP_LIK_GAUSSIAN   scripts/svgp.py:127-200,207-233 and scripts/hurdle.py:127-252 (regression; noise variance)
 *   ZIGP_LIK_BERNOULLI  scripts/classifier.py:116-240 (log probit(fmean / sqrt(1 + fvar)) of the 0/1 label, y == 1 is "on")
 * Only the f fields of zigp_kron_params / zigp_kron_grads are read / written (g pointers may be NULL; noise is ignored
 * by the Bernoulli head).  f_mu is the constant mean offset of classifier.py:70-72,136-137 (0 when include_f_mu is False);
 * d_f_mu (nullable) receives the gradient of the scaled data term with respect to it. */
#define ZIGP_LIK_ONOFF 0
#define ZIGP_LIK_GAUSSIAN 1
#define ZIGP_LIK_BERNOULLI 2
int zigp_kron_head_elbo(zigp_ctx* ctx, const zigp_kron_params* p, int32_t lik, const double* X, const double* Y,
                        int64_t N, double jitter, double scale, double f_mu, int32_t include_kl,
                        double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu);
/* The same bound on rows [row_begin, row_end) of the RESIDENT data set (zigp_set_data / zigp_set_data_device, D = D0 + D1): the
 * single-latent companion of zigp_kron_elbo_rows -- no minibatch upload, same numbers as zigp_kron_head_elbo on those rows; grids beyond
 * the fused kernels take the panel path with a device-to-device copy of the rows, an empty range is a zero data term. */
int zigp_kron_head_elbo_rows(zigp_ctx* ctx, const zigp_kron_params* p, int32_t lik, int64_t row_begin, int64_t row_end,
                             double jitter, double scale, double f_mu, int32_t include_kl,
                             double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu);

/* The Adam fit loop of the heads on the device: replaces the training loops of scripts/svgp.py:240-330, scripts/classifier.py:276-316 and
 * the regression loop of scripts/hurdle.py (its classifier loop is classifier.py's) for n_steps consecutive iterations -- the gradient of
 * cost = -(scale * sum var_exp - KL), the Log1pe chain and one Adam per learning rate run in kernels, the steps are enqueued back to back
 * and the host synchronises once per call.  Call semantics are those of zigp_kron_fit_steps, word for word (shape: sizes M0f, M1f, D0, D1
 * only; free_state / adam_m / adam_v in/out; t0; row_begin[i] >= 0 selects rows of the resident set, -(1 + k) host batch k of Xw / Yw;
 * elbo_data / kl are the history, each entry taken BEFORE its step's update; a Cholesky failure in step k returns ZIGP_ENOTPD with the
 * state before that step, NaN history from k on and k in zigp_kron_fit_steps_applied -- the two fit loops share that counter; a
 * communicator is honoured as there).  Block order of free_state (ZIGP_HEAD_FIT_BLOCKS = 10, all always present, so n_free =
 * M0 D0 + M1 D1 + 2 M0 M1 + D0 + D1 + 4): Z0 (M0 x D0), Z1 (M1 x D1), u_m (M0 M1), u_s_sqrt (M0 M1), ell0 (D0), ell1 (D1), var0, var1,
 * noise (ignored by the Bernoulli head), f_mu (the constant of classifier.py:70-72,136-137).  A block with trainable = 0 keeps its x, m, v;
 * its value is the transform of its free entry: an absent f_mu is an untrainable block with free value 0, the classifier's noise an
 * untrainable block with any positive value.
 * ZIGP_EARG, with nothing enqueued and the state untouched: lik neither ZIGP_LIK_GAUSSIAN nor ZIGP_LIK_BERNOULLI, a grid beyond the
 * fused kernels (step it with zigp_kron_head_elbo_rows and a host optimiser), a wrong n_free, a row range outside the resident set, NULL
 * arguments, bad Adam constants. */
#define ZIGP_HEAD_FIT_BLOCKS 10
typedef struct {
  double lr[ZIGP_HEAD_FIT_BLOCKS];          /* Adam learning rate of each block */
  int32_t positive[ZIGP_HEAD_FIT_BLOCKS];   /* 1: value = log(1 + exp(x)) + 1e-6 (Log1pe), 0: value = x */
  int32_t trainable[ZIGP_HEAD_FIT_BLOCKS];  /* 0: the block is not updated */
  double beta1, beta2, eps;                 /* TensorFlow's defaults: 0.9, 0.999, 1e-8 */
} zigp_kron_head_fit_opts;
int zigp_kron_head_fit_steps(zigp_ctx* ctx, const zigp_kron_params* shape, int32_t lik, const zigp_kron_head_fit_opts* opts,
                             double* free_state, double* adam_m, double* adam_v, int64_t n_free,
                             int64_t t0, int32_t n_steps, const int64_t* row_begin, int64_t batch,
                             const double* Xw, const double* Yw, double jitter, double scale, int32_t include_kl,
                             double* elbo_data, double* kl);

/* Replaces predict_svgp / predict_scgp (onofftf/svgppred.py:15-203, onofftf/svcppred.py:15-224).  out4 = 4 x N rows:
 * fmean, fvar, pfmean, pfvar.  Bernoulli: pfmean = probit(fmean / sqrt(1 + fvar)), pfvar = pfmean - pfmean^2
 * (svcppred.py "pfmean"/"pfvar"); Gaussian: pfmean = fmean, pfvar = fvar + noise (svgppred.py returns rows 0-1). */
int zigp_kron_head_predict(zigp_ctx* ctx, const zigp_kron_params* p, int32_t lik, const double* Xnew, int64_t N,
                           double jitter, double f_mu, double* out4);

/* ---- heads on the dense path: the same two baselines on the dense engine (scattered inputs, any D up to ZIGP_MAX_D, Matern kernels) ----
 * GPflow 0.4.0's SVGP with likelihoods.Gaussian / likelihoods.Bernoulli: latent f alone under
 *   ZIGP_LIK_GAUSSIAN   ve = -1/2 log 2pi - 1/2 log noise - 1/2 ((y - fm)^2 + fv) / noise            (scripts/svgp.py:198-200)
 *   ZIGP_LIK_BERNOULLI  p = probit(fm / sqrt(1 + fv)) (1 - 2e-3) + 1e-3, ve = log(y == 1 ? p : 1 - p)   (scripts/classifier.py:139-140,210-217)
 * in the arithmetic of the Kronecker heads' point-wise kernel.  lik belongs to the call: no context switch, no other call changes.
 * Read: Mf, D, Zf, u_fm, u_fs_sqrt, ell_f, var_f and noise (Bernoulli ignores noise; its gradient comes back 0).  Mg and the g pointers are
 * not read and may be 0 / NULL.  Written: the f fields and noise of grads (the g fields are left alone); *kl = KL_f, or 0 when include_kl is 0.
 * Everything zigp_elbo / zigp_predict honour for latent f holds: the resident data, zigp_select_rows and row ranges, zigp_set_whiten and
 * zigp_set_q_full (u_fs_sqrt and its gradient (Mf, Mf)), zigp_set_kernel(ctx, 0, kind), zigp_set_mean_function /
 * zigp_get_mean_function_grad, D up to ZIGP_MAX_D under the same rules (Matern and Linear at D <= 8), zigp_set_chunk and zigp_set_overlap.
 *
 * HOW IT RUNS, AND WHAT THAT COSTS.  The chunk loop of the dense path is a two-latent schedule (paired tile lists, merged launches).  A head
 * call runs that schedule as it is: the second latent is a library-owned PLACEHOLDER -- one inducing point at the origin, u = 0, s = 1
 * (L_q = [1] with zigp_set_q_full), ell = 1 and var = 1 in every dimension, RBF whatever zigp_set_kernel(ctx, 1, ...) holds -- and only the
 * point-wise launch differs (k_pointwise_head reads the planes of f and writes zero cotangents for the placeholder, so the placeholder's
 * data gradient is exactly zero).  Its KL and its gradient blocks are dropped when the result is gathered.  The cost: the placeholder pads
 * to one 128-row panel, so (128 / Mp)^2 of latent f's matrix work (Mp = Mf rounded up to 128) rides along, plus its launches -- about half
 * an OnOff step with Mg = Mf, plus that share.  A one-latent schedule is a later change.
 * ZIGP_EARG, naming the argument, with nothing enqueued and every output untouched: lik neither ZIGP_LIK_GAUSSIAN nor ZIGP_LIK_BERNOULLI;
 * what zigp_elbo refuses for the f half of params; a communicator attached (zigp_comm_init: the heads are single-process).
 * Not covered: zigp_fit_steps[_mode] (fit with zigp_head_elbo and a host optimiser), zigp_sample_paths, zigp_predict_density /
 * zigp_predict_scores (zigp_density_rows / zigp_score_rows take rows 0-1 of zigp_head_predict with the same lik). */
int zigp_head_elbo(zigp_ctx* ctx, const zigp_params* p, int32_t lik, double jitter, double scale, int64_t row_begin, int64_t row_end,
                   int32_t include_kl, double* elbo_data, double* kl, zigp_grads* grads);
/* out4 = 4 x N rows in the order of zigp_kron_head_predict: fmean, fvar, pfmean, pfvar (Gaussian: fmean, fvar + noise; Bernoulli: p,
 * p - p^2).  The _device form takes and fills device memory of the context's GPU and is complete on return. */
int zigp_head_predict(zigp_ctx* ctx, const zigp_params* p, int32_t lik, const double* Xnew, int64_t N, double jitter, double* out4);
int zigp_head_predict_device(zigp_ctx* ctx, const zigp_params* p, int32_t lik, const double* dXnew, int64_t N, double jitter,
                             double* d_out4);

/* ---- predictive density of held-out data and the moments of y (new: the reference's likelihood leaves them out -- "not implemented
 * logp, conditional_mean and others", onoffgpf/OnOffLikelihood.py:28; GPflow's predict_density / predict_y) ----
 * OnOff: at a test row f ~ N(fm, fv) and g ~ N(gm, gv) are independent under q (rows 3-6 of zigp_predict, mean
 * function and g_offset applied) and y | f, g ~ N(Phi~(g) f, noise), Phi~(g) = 0.5 (1 + erf(g / sqrt 2)) (1 - 2e-3) + 1e-3
 * (OnOffSVGP.py:178).  f integrates out in closed form, g by the caller's rule for the standard normal -- nodes x_i, weights w_i > 0
 * with sum w_i = 1, n_quad <= ZIGP_DENSITY_MAX_QUAD of them:
 *   Phi_i = Phi~(gm + sqrt(max(gv, 0)) x_i),   s_i = noise + Phi_i^2 max(fv, 0),
 *   logp  = logsumexp_i [ log w_i - 0.5 log(2 pi s_i) - 0.5 (y - Phi_i fm)^2 / s_i ].
 * This finite sum IS the result; how far it lies from the integral is a property of the rule (Gauss-Hermite with 64 nodes is the Python
 * default; a row whose mass sits in the far tail of q(g) is beyond any rule centred on gm -- DESIGN.md section 10).
 *   ymean = gfmean,  yvar = (gfvar + gfmeanu) + noise   (rows 0-2 of zigp_predict; the two additions in that order).
 * Heads, closed form: ZIGP_LIK_GAUSSIAN  logp = log N(y; fm, fv + noise), ymean = fm, yvar = fv + noise;
 *                     ZIGP_LIK_BERNOULLI p = pfmean of zigp_kron_head_predict (probit(fm / sqrt(1 + fv)) through the same link),
 *                                        logp = log p for y == 1 and log1p(-p) otherwise, ymean = p, yvar = p (1 - p).
 * out3 (nullable in all three calls) is (3, N): logp, ymean, yvar.  *sum receives sum_n logp_n, added in a fixed order (the same bits
 * on every call).  N = 0 is ZIGP_OK with *sum = 0.
 * ZIGP_EARG, with nothing enqueued, the outputs untouched and the context usable afterwards: a NULL context, an unknown lik, N < 0,
 * noise not positive (the Bernoulli head ignores noise), a NULL sum or row pointer, and for OnOff n_quad outside
 * [1, ZIGP_DENSITY_MAX_QUAD], NULL nodes or weights, a non-finite node, a weight that is not positive and finite. */
#define ZIGP_DENSITY_MAX_QUAD 256
/* Rows in HOST memory, for the Kronecker path and the heads: feed it the rows of zigp_kron_predict (3-6) or zigp_kron_head_predict
 * (0-1).  gm, gv, nodes and weights are ignored for the heads and may be NULL there.  OnOff computes gfmean, gfvar and gfmeanu from
 * the four rows as zigp_predict does. */
int zigp_density_rows(zigp_ctx* ctx, int32_t lik, const double* fm, const double* fv, const double* gm, const double* gv,
                      const double* y, int64_t N, double noise, const double* nodes, const double* weights, int32_t n_quad,
                      double* out3, double* sum);
/* Dense path: zigp_predict into the context's own (9, N) block, then the density kernel over it; only out3 and the sum come back.
 * Every parametrisation, kernel kind, mean function and D that zigp_predict accepts (it consumes nothing but its rows), and
 * zigp_predict's errors (ZIGP_ENOTPD included).  Xnew (N, D), Ynew (N), out3 (3, N) in host memory. */
int zigp_predict_density(zigp_ctx* ctx, const zigp_params* p, const double* Xnew, const double* Ynew, int64_t N, double jitter,
                         double g_offset, const double* nodes, const double* weights, int32_t n_quad, double* out3, double* sum);
/* The same with Xnew, Ynew and out3 in DEVICE memory of the context's GPU (the companion of zigp_predict_device; anything else is
 * ZIGP_EARG): nothing crosses PCIe but the parameters, the rule (host pointers) and the sum (a host double); complete on return. */
int zigp_predict_density_device(zigp_ctx* ctx, const zigp_params* p, const double* dXnew, const double* dYnew, int64_t N, double jitter,
                                double g_offset, const double* nodes, const double* weights, int32_t n_quad, double* d_out3, double* sum);
/* The same rule centred on each row's mode (OnOff only; DESIGN.md section 10, "centred").  A rule centred on gm cannot see mass that
 * sits far from gm or in a spike between its nodes; these three calls shift and scale the caller's rule, per row, to a mode of the
 * integrand.  With sg = sqrt(max(gv, 0)), z = (g - gm) / sg,
 *   F(z) = -z^2 / 2 + l(Phi~(gm + sg z)),   l(u) = -0.5 log(2 pi s(u)) - 0.5 (y - u fm)^2 / s(u),   s(u) = noise + u^2 max(fv, 0):
 *   zhat = a local maximiser of F: a safeguarded Newton search from z = 0 with analytic derivatives (every step at most one unit of g and
 *          halved until F does not decrease; at most 60 iterations),  tau = 1 / sqrt(-F''(zhat)) clamped to (0, 1.5], 1 where -F'' <= 0;
 *   z_i  = zhat + tau x_i,
 *   logp = logsumexp_i [ log w_i + x_i^2 / 2 + log tau - z_i^2 / 2 + l(Phi~(gm + sg z_i)) ].
 * Given (zhat, tau) that finite sum IS the result (one node: the Laplace approximation); gv <= 0 gives zhat = 0, tau = 1 exactly.
 * centre2 (nullable) is (2, N): zhat, tau -- host memory, device memory in the _device call.  ymean, yvar, *sum, out3, the
 * refusals and every other argument are those of the call without the suffix, bit for bit where they do not depend on the rule. */
int zigp_density_rows_centred(zigp_ctx* ctx, const double* fm, const double* fv, const double* gm, const double* gv, const double* y,
                              int64_t N, double noise, const double* nodes, const double* weights, int32_t n_quad, double* out3,
                              double* sum, double* centre2);
int zigp_predict_density_centred(zigp_ctx* ctx, const zigp_params* p, const double* Xnew, const double* Ynew, int64_t N, double jitter,
                                 double g_offset, const double* nodes, const double* weights, int32_t n_quad, double* out3, double* sum,
                                 double* centre2);
int zigp_predict_density_centred_device(zigp_ctx* ctx, const zigp_params* p, const double* dXnew, const double* dYnew, int64_t N,
                                        double jitter, double g_offset, const double* nodes, const double* weights, int32_t n_quad,
                                        double* d_out3, double* sum, double* d_centre2);

/* ---- predictive scores: CDF, quantiles and CRPS of y (new) ----
 * The predictive distribution of y at a test row is the finite Gaussian mixture of the density above (the rule centred on gm):
 *   mu_k = Phi_k fm,   s_k = noise + Phi_k^2 max(fv, 0),   z_k(t) = (t - mu_k) / sqrt(s_k),   Phi_k as in zigp_density_rows;
 *   F(t)  = sum_k w_k Phi(z_k(t)),   SF(t) = sum_k w_k Phi(-z_k(t)),   Phi(z) = erfc(-z / sqrt 2) / 2  -- each its own sum, never
 *           1 - the other, so that the small tail keeps its relative accuracy;
 *   quantile at p in (0, 1): the t with F(t) = p, found by a bracketed Newton search on F = p (p <= 1/2) or SF = 1 - p (p > 1/2) that
 *           starts from [min_k, max_k] of mu_k + sqrt(s_k) Phi^-1(p) and ends on a bracket one ulp wide or a step that changes nothing;
 *   CRPS  = sum_i w_i A(y - mu_i, s_i) - 1/2 sum_i sum_j w_i w_j A(mu_i - mu_j, s_i + s_j),
 *           A(m, v) = 2 sqrt(v) phi(m / sqrt v) + m (2 Phi(m / sqrt v) - 1)     (the closed form for a Gaussian mixture).
 * These finite sums ARE the results, as the density's sum is.  ZIGP_LIK_GAUSSIAN is the one-component case mu = fm, s = fv + noise:
 * F = Phi(z), quantile = fm + sqrt(s) Phi^-1(p), CRPS = A(y - fm, s) - sqrt(s / pi).  ZIGP_LIK_BERNOULLI has no density and is refused
 * by name: its CRPS is the Brier score (ymean - y)^2 of zigp_density_rows.
 * The rule is the fixed one only: a rule that moves with y (the _centred calls) does not define one distribution per row.
 * Outputs, each nullable and computed only when asked for: cdf2 (2, N): F(y), SF(y); quant (n_levels, N): one row per level, in the
 * caller's order (any order, duplicates allowed); crps (N); *crps_sum = sum_n CRPS_n, added in a fixed order (the same bits on every
 * call).  y (Ynew) may be NULL, and then cdf2, crps and crps_sum must be NULL; n_levels = 0 goes with NULL levels and quant.
 * N = 0 is ZIGP_OK with *crps_sum = 0.
 * ZIGP_EARG, with nothing enqueued, the outputs untouched and the context usable afterwards: a NULL context (before anything else is
 * read), the Bernoulli head, what zigp_density_rows refuses of lik, N, noise, n_quad and the rule, n_levels outside
 * [0, ZIGP_SCORE_MAX_LEVELS], a level that is not finite and strictly inside (0, 1), NULL levels or quant with n_levels > 0 (or
 * either given with n_levels = 0), a NULL y with cdf2, crps or crps_sum given, a NULL row pointer. */
#define ZIGP_SCORE_MAX_LEVELS 16
/* Rows in HOST memory, for the Kronecker path and the Gaussian head: rows 3-6 of zigp_kron_predict or 0-1 of zigp_kron_head_predict.
 * gm, gv, nodes and weights are ignored for the Gaussian head and may be NULL there. */
int zigp_score_rows(zigp_ctx* ctx, int32_t lik, const double* fm, const double* fv, const double* gm, const double* gv,
                    const double* y, int64_t N, double noise, const double* nodes, const double* weights, int32_t n_quad,
                    const double* levels, int32_t n_levels, double* cdf2, double* quant, double* crps, double* crps_sum);
/* Dense path: zigp_predict into the context's own (9, N) block, then the score kernel over its rows 3-6; only what was asked for comes
 * back.  Every parametrisation, kernel kind, mean function and D that zigp_predict accepts, and zigp_predict's errors (ZIGP_ENOTPD
 * included).  Xnew (N, D), Ynew (N) and the outputs in host memory. */
int zigp_predict_scores(zigp_ctx* ctx, const zigp_params* p, const double* Xnew, const double* Ynew, int64_t N, double jitter,
                        double g_offset, const double* nodes, const double* weights, int32_t n_quad, const double* levels,
                        int32_t n_levels, double* cdf2, double* quant, double* crps, double* crps_sum);
/* The same with Xnew, Ynew, cdf2, quant and crps in DEVICE memory of the context's GPU (anything else is ZIGP_EARG); the rule, the
 * levels and crps_sum stay host pointers; complete on return. */
int zigp_predict_scores_device(zigp_ctx* ctx, const zigp_params* p, const double* dXnew, const double* dYnew, int64_t N, double jitter,
                               double g_offset, const double* nodes, const double* weights, int32_t n_quad, const double* levels,
                               int32_t n_levels, double* d_cdf2, double* d_quant, double* d_crps, double* crps_sum);

/* ---- sample paths: joint posterior draws at test inputs by pathwise conditioning (new) ----
 * Replaces GPflow 0.4.0's predict_f_samples for the model that OnOffSVGP mirrors, without a T x T covariance: a path is
 *   f*(x) = f_prior(x) + k(x, Z) Kuu^-1 (u - f_prior(Z)),   u ~ q(u),   f_prior a random-feature draw of the prior (Wilson et al., 2020),
 * so every test row is one finite sum given the draw.  Per latent h, row n and sample s, THE definition:
 *   out[h][s][n] = shift_h + sum_d lin_h[d] x[n][d] + sum_{m<M} V_h[m][s] k_h(x_n, z_m)
 *                + sum_{r<R} amp_h[r][s] cos( sum_d omega_h[r][d] x[n][d] + phase_h[r] )
 * k_h the latent's ZIGP_KERN_* kind with the Kuf panel's own element function (the Matern kinds through the floored distance
 * sqrt(r^2 + 1e-12)).  One summation order per element (kernel terms in groups of four in ascending m, then the cosines in ascending r,
 * the mean part last): an element's bits do not depend on N, on the row's position, on S, on the sample's column, on the other latent
 * or on the call.  1 <= D <= 8, 1 <= S <= ZIGP_PATH_MAX_S, M >= 1, R >= 0 (R = 0: the conditional-mean part alone).  The cosine is
 * correct for every finite argument; beyond the library's fast range (|argument| of about 1e5 and more) it takes a slower path.
 * ZIGP_EARG with a message that names the argument, nothing enqueued and the context usable afterwards: D > 8 (the message names D),
 * S outside [1, 256], R < 0, M < 1, an unknown kind, a NULL table, a non-finite table entry, and a host pointer handed to a _device call.
 * The Kronecker path and its heads draw their paths through the entry points of zigp_kronpaths.h; D > 8 has none. */
#define ZIGP_PATH_MAX_S 256
typedef struct {
  int32_t kind, M, R, reserved;      /* ZIGP_KERN_*, inducing points, random features */
  const double* Z;                   /* (M,D) */
  const double* ell;                 /* (D) */
  double var;
  const double* V;                   /* (M,S) weights of the kernel terms */
  const double* omega;               /* (R,D) frequencies */
  const double* phase;               /* (R) */
  const double* amp;                 /* (R,S) weights of the cosines */
  const double* lin;                 /* (D) or NULL */
  double shift;
} zigp_path_latent;
/* The sum above and nothing else.  lat: nlat (1 or 2) records, all arrays in host memory; X (N,D) and out (nlat,S,N) in host memory. */
int zigp_path_rows(zigp_ctx* ctx, const zigp_path_latent* lat, int32_t nlat, int32_t D, int32_t S, const double* X, int64_t N, double* out);
/* The same with X and out in DEVICE memory of the context's GPU (the tables stay host pointers); complete on return. */
int zigp_path_rows_device(zigp_ctx* ctx, const zigp_path_latent* lat, int32_t nlat, int32_t D, int32_t S, const double* dX, int64_t N,
                          double* d_out);
/* A parameter-free draw of one latent: R random features and the standard normals behind u.  Handing the same draw to calls with other
 * inputs or other hyperparameters gives the same paths there. */
typedef struct {
  int32_t R, reserved;
  const double* omega0;              /* (R,D) frequencies for unit lengthscales: N(0, I) for RBF, Student-t with 2 nu degrees for Matern */
  const double* phase;               /* (R) uniform on [0, 2 pi) */
  const double* a;                   /* (R,S) standard normals */
  const double* eps;                 /* (M,S) standard normals */
} zigp_path_draw;
/* Joint sample paths of the dense OnOff model.  Per latent: omega = omega0 / ell, amp = a sqrt(2 var / R); f_Z = the sum above at the
 * rows Z with V = 0; V = W^T t with the W = L^-1 of the call's own M x M forward stage (Kuu + jitter I = L L^T) and
 *   unwhitened: t = W (u_m + s o eps - f_Z), then one step of iterative refinement of V against Kuu;
 *   whitened (zigp_set_whiten): t = u_m + s o eps - W f_Z;
 *   whitened, full covariance (zigp_set_q_full): t = u_m + tril(L_q) eps - W f_Z;
 * then the sum at Xnew, with the context's mean function (zigp_set_mean_function) as lin and shift of f and g_offset as the shift of g,
 * as rows fmean and gmean of zigp_predict carry them.  Honours zigp_set_kernel.  out3 is (3,S,N): f, g, and gf = Phi~(g) f with the link
 * of the predictive density.  zigp_predict's errors (ZIGP_ENOTPD included) and the refusals above. */
int zigp_sample_paths(zigp_ctx* ctx, const zigp_params* p, const double* Xnew, int64_t N, double jitter, double g_offset,
                      const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* out3);
/* The same with Xnew and out3 in DEVICE memory of the context's GPU; the draws stay host pointers; complete on return. */
int zigp_sample_paths_device(zigp_ctx* ctx, const zigp_params* p, const double* dXnew, int64_t N, double jitter, double g_offset,
                             const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* d_out3);

/* ---- Kronecker sample paths: the same draws for the Kronecker (space x time) model and its heads (new).
 * Their record and entry points are declared in zigp_kronpaths.h, which is part of this boundary. */
#include "zigp_kronpaths.h"

/* ---- sample-path scores: group totals, energy and variogram scores of an ensemble (new).  Their options record
 * and entry points are declared in zigp_ensemble.h, which is part of this boundary. */
#include "zigp_ensemble.h"

/* ---- inducing inputs by k-means on the device: Lloyd iterations (new entry points) ----
 * Replaces the host-side scipy.cluster.vq.kmeans call that picks the inducing inputs before the first ELBO step (scripts/onoff.py:67,
 * scripts/svgp.py:64; the same call in onofftf/model.py init_params and onofftf/heads.py init_head_params) by its Lloyd iterations from a
 * start the caller chooses; seeding, restarts and a tolerance stop stay with the caller.  THE definition -- X: N rows of stride ld doubles,
 * of which the D columns from col0 are used; C (M, D) row-major, read and written.  Iteration t = 1, 2, ... with the current C:
 *   d(i, j)   = sum_k (x_ik - c_jk)^2, k ascending, in the difference form (never |x|^2 - 2 x.c + |c|^2);
 *   label_i   = the LOWEST j attaining min_j d(i, j);
 *   c_j      <- (sum of the rows of label j) / count_j where count_j > 0; an empty cluster keeps its centroid;
 *   inertia_t = sum_i d(i, label_i) against C before the update;  changed_t = rows whose label differs from iteration t - 1, changed_1 = N.
 * The loop stops after the first t with changed_t = 0 (that iteration's update reproduces C bit for bit), or at t = max_iter.
 * Outputs: C; labels int32 [N] of the last assignment; counts int64 [M]; history double [max_iter][2] = (inertia_t, changed_t), rows past
 * *n_iter left as the caller passed them; *n_iter.  labels, counts and history may be NULL.  Every sum has one fixed order (no
 * floating-point atomics): the same call gives the same bits every time, and the three forms below agree bit for bit on the same rows.
 * Limits: 1 <= D <= ZIGP_MAX_D, 1 <= M <= min(N, ZIGP_KMEANS_MAX_M), N < 2^31, 1 <= max_iter <= 1048576.
 * ZIGP_EARG with a message that names the argument, the outputs untouched and the context usable afterwards: a NULL context (before
 * anything else is read), M < 1, M > N, M > ZIGP_KMEANS_MAX_M, D out of range, col0 < 0 or col0 + D > ld, max_iter out of range, a NULL
 * X, C or n_iter, no resident data (the _resident form), a host pointer handed to the _device form (refused, not dereferenced), a
 * non-finite entry of C (checked on the host: a NaN centroid never wins a row) and an inertia of iteration 1 that is not finite (X
 * holds a non-finite value in the columns used). */
#define ZIGP_KMEANS_MAX_M 4096
/* X (N, ld), C and the outputs in HOST memory. */
int zigp_kmeans(zigp_ctx* ctx, const double* X, int64_t N, int32_t ld, int32_t col0, int32_t D, int32_t M, double* C, int32_t max_iter,
                int32_t* labels, int64_t* counts, double* history, int32_t* n_iter);
/* The same with X in DEVICE memory of the context's GPU (e.g. a torch tensor); C and the outputs stay host pointers. */
int zigp_kmeans_device(zigp_ctx* ctx, const double* dX, int64_t N, int32_t ld, int32_t col0, int32_t D, int32_t M, double* C,
                       int32_t max_iter, int32_t* labels, int64_t* counts, double* history, int32_t* n_iter);
/* The same on the WHOLE resident set of zigp_set_data / zigp_set_data_device (ld = its D): a selection made by zigp_select_rows is
 * ignored and left as it was. */
int zigp_kmeans_resident(zigp_ctx* ctx, int32_t col0, int32_t D, int32_t M, double* C, int32_t max_iter, int32_t* labels, int64_t* counts,
                         double* history, int32_t* n_iter);

/* ---- data-parallel exchange (new: the reference is single-process) ----
 * The ELBO data term is a sum over points (tf.reduce_sum(var_exp), onoffgpf/OnOffSVGP.py:122; scripts/onoff.py:307): one process per GPU
 * holds a row shard, and ONE ncclAllReduce(sum, f64) per step adds the packed [elbo_data, kl, gradient] vector of every rank, on the
 * device, on the library's stream (RCCL over xGMI; ~82 KB at M = 1024, D = 3).  RCCL is bound at run time (librccl.so.1).
 *   rank 0:      zigp_comm_unique_id(id)  -> send the 128 bytes to the other ranks by any means (torch.distributed broadcast, MPI, a file)
 *   every rank:  zigp_comm_init(ctx, rank, nranks, id)       (collective: returns when all ranks have joined)
 * From then on zigp_elbo, zigp_kron_elbo, zigp_kron_elbo_rows, zigp_kron_head_elbo and zigp_kron_head_elbo_rows return the SUM over ranks of elbo_data, kl, grads
 * (and d_f_mu, the mean-function gradient) on every rank: each rank passes its own rows and include_kl = (rank == 0), so that the KL
 * and its gradient are counted once.  Every rank must make the same calls in the same order with the same model sizes.  Prediction
 * entry points are unaffected.  A Cholesky failure is reported by every rank (their Kuu are identical), after the exchange. */
#define ZIGP_COMM_ID_BYTES 128
int zigp_comm_unique_id(void* id /* [ZIGP_COMM_ID_BYTES] */);
int zigp_comm_init(zigp_ctx* ctx, int32_t rank, int32_t nranks, const void* id);
/* ZIGP_OK when RCCL can be bound in this process (librccl.so.1 found, every symbol resolved, an NCCL 2.x version of the same major as
 * the headers the library was built against); *version (nullable) = its ncclGetVersion code.  Ranks should agree on this BEFORE any of
 * them enters the collective zigp_comm_init: a rank that cannot load RCCL would otherwise leave its peers waiting. */
int zigp_comm_available(int32_t* version);
/* zigp_comm_init gives up with ZIGP_ECOMM when its peers have not joined after `seconds` (default 120, or env ZIGP_COMM_TIMEOUT_S at
 * zigp_create); the communicator is then unusable on every rank: fall back to a host-side exchange or exit, do not retry on the same id.
 * The helper thread that is still inside ncclCommInitRank stays behind (it destroys the communicator itself should the call return late):
 * a process that goes on after a timeout should end through os._exit / a fresh child process rather than a normal interpreter shutdown. */
int zigp_comm_set_timeout(zigp_ctx* ctx, double seconds);
int zigp_comm_destroy(zigp_ctx* ctx);
/* Sum n host doubles over the ranks of the context's communicator, in place (staged through the device): for the few scalars a host loop
 * wants agreed on (a convergence flag, a timing), and the self-check the Python wrapper runs right after zigp_comm_init. */
int zigp_comm_allreduce_host(zigp_ctx* ctx, double* inout, int64_t n);
/* rank / nranks of the context's communicator (nranks = 0: none) and the number of all-reduces issued through it so far */
int zigp_comm_info(zigp_ctx* ctx, int32_t* rank, int32_t* nranks, int64_t* allreduce_calls);

/* Stream overlap inside zigp_elbo (default ON since round 3): the HBM-bound kernels of a row chunk (Kuf-cotangent reductions,
 * the next chunk's Kuf panels) run on a second HIP stream underneath the chunk's two MFMA-bound rank-N updates (-3 % per
 * cfg3 step), and (round 5) the point-wise stage of a gradient step rides as the leading workgroups of the launch of the J' product,
 * which does not depend on it (one launch boundary less per chunk).  Results are bit-identical either way.  Turn it off (0) to profile:
 * every kernel then runs alone, under its own name, on one stream and per-kernel durations from an external tracer (rocprofv3 --stats) mean
 * what they say; the library's own event timing (zigp_profile_*, include/zigp_diag.h) already keeps the chunks it times that way. */
int zigp_set_overlap(zigp_ctx* ctx, int32_t on);

#ifdef __cplusplus
}
#endif
#endif
