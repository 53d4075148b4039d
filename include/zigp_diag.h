/* libzigp -- measurement hooks (bench.py) and diagnostics used by the parity tests.  Not part of the drop-in boundary
 * (include/zigp.h); exported by the same libzigp.so. */
#ifndef ZIGP_DIAG_H
#define ZIGP_DIAG_H
#include "zigp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement hooks (bench.py) ---- */
/* Accumulated HIP-event time (ms), launch count and algorithmic flops per kernel class since the last reset,
 * measured with HIP events on the stream the kernels run on.  Classes (gemm_f64_kernel template arguments are
 * <A layout, B layout, ring stages, k-scale, triangular mode, waves, epilogue>):
 * 0 gemm_A1  A1 = W K                  gemm_f64_kernel<1,1,2,false,1,8,EpiStoreColsum>   (W read through its transpose; fused sum v A1, sum A1^2)
 * 1 gemm_A2  A2 = W^T A1               gemm_f64_kernel<1,1,2,false,2,8,EpiColsum>        (fused sum s^2 A2^2; the panel itself is not stored;
 *                                      value-only ELBO and predict only: a gradient step takes the variance from class 3)
 * 2 gemm_H   (not launched since round 4: H = W diag(s^2) A2 is folded into class 3; the slot keeps the class numbering)
 * 3 gemm_J   J' = Q A2 = (Q W^T) A1    gemm_f64_kernel<1,1,2,false,0,8,EpiStorePanelKColsum>  (one full product on the A1 panel; fused
 *                                      sum_m K J' = sum s^2 A2^2 - sum A1^2, the variance term of a gradient step)
 * 4 syrk     C1 += A1 G A1^T           gemm_f64_kernel<0,0,2,true,3,4,EpiAccum>
 * 5 kuf_build   6 pointwise   7 kgrad   8 MxM stage (all kernels)   9 everything else.
 * Whitened calls (zigp_set_whiten) book their launches in the same classes: 0 gemm_A1  A = W K with the weights u and s^2 - 1
 * (<1,1,2,false,1,8,EpiStoreColsum> in a gradient step, <1,1,2,false,1,8,EpiColsum> -- no panel stored -- otherwise), 3 gemm_J
 * J' = (W^T D) A, gemm_f64_kernel<1,1,2,false,2,8,EpiStore>, with M^2 Nc flops per latent; class 1 is not launched. */
#define ZIGP_NCLASS 10
int zigp_profile_enable(zigp_ctx* ctx, int32_t on);
int zigp_profile_get(zigp_ctx* ctx, double* ms /*[ZIGP_NCLASS]*/, int64_t* launches /*[ZIGP_NCLASS]*/,
                     double* flops /*[ZIGP_NCLASS] algorithmic*/);
int zigp_profile_reset(zigp_ctx* ctx);
/* Event pairs cost ~10 us each, so launches of the chunk loop are TIMED on every 8th full-size chunk only (ms / launches /
 * flops above describe those sampled launches); zigp_profile_totals returns the number of launches per class, sampled or not. */
int zigp_profile_totals(zigp_ctx* ctx, int64_t* total_launches /*[ZIGP_NCLASS]*/);
/* every = 1: time EVERY launch of the chunk loop, the partial last chunk included (sums are then exact, the step is ~1 % slower:
 * bench.py's separate profiled pass); every = n > 1: full-size chunks only, every n-th (default 8). */
int zigp_profile_sampling(zigp_ctx* ctx, int32_t every);

/* Clock stamps of the 8 XCDs, taken in stream order on the library's main stream (the call synchronises): out[8][3] =
 * {XCC id, shader-clock counter (s_memtime), constant 100 MHz counter (s_memrealtime)}.  Two calls around a region give the
 * sustained shader clock of that region: (cycles_1 - cycles_0) / ((rt_1 - rt_0) / 1e8), paired by XCC id. */
int zigp_clock_stamp(zigp_ctx* ctx, int64_t* out /*[24]*/);

/* ---- diagnostics used by the parity tests (building blocks through the same kernels) ---- */
/* Kronecker entry points: on != 0 forces the GEMM-panel path (zigp_kron.hip) also for grids the fused register-resident kernels
 * (zigp_kronf.hip) cover -- two independent implementations of the same factored algebra that the tests check against each other. */
int zigp_set_kron_panels(zigp_ctx* ctx, int32_t on);
/* Host only -- no context, no GPU: builds the tile lists the chunk loop launches for its triangular products (lower: A1 = W K, else
 * A2 = W^T A1) of a chunk of Nc rows (a multiple of 128) with Mf / Mg inducing points, exactly as chunk_forward does (paired order, merged
 * launch, LPT tail of a last wave that is not full when tail_on), and checks them: every (row block, column panel) tile exactly once, with
 * the whole k range of its row block.  out[8] = {workgroups of latent f's list, of latent g's, entries per workgroup f, g, tail units f, g,
 * largest tail workgroup in k blocks, paired order (0 / 1)}.  Returns 0, ZIGP_EARG, or -10 ... -13 for a list that is not a partition. */
int zigp_test_trmm_list(int32_t lower, int32_t Mf, int32_t Mg, int64_t Nc, int32_t tail_on, int64_t* out);
/* Host only (no context, no GPU): the tile list of the moments product of the wide Kuf gradient (input dimensions 9 .. ZIGP_MAX_D) as
 * zigp_elbo plans it for M inducing points and a chunk of Nc rows (a multiple of 1024).  out[0] = split-K slices, out[1] = list entries
 * per workgroup, out[2] = entries, then (bi, bj, kbeg, kend, slice) per entry (k in units of 16 rows), as many entries as fit `cap`
 * int64 values.  Returns 0 or ZIGP_EARG. */
int zigp_test_kgmom_list(int32_t M, int64_t Nc, int64_t cap, int64_t* out);
/* Host only (no context, no GPU): the split-K tile list of one of the eight k-range rules of the dense M x M stages (SkRule, csrc/zigp_host.h:
 * 0 "s", 1 "y", 2 "r", 3 "tt", 4 "full", 5 "t", 6 "rt", 7 "rfull") for an nb x nb block product, from the one builder the launcher uploads
 * from.  out[0] = split-K slices, out[1] = whether the rule's finish pass is lower_only (tiles above the diagonal are not computed and are
 * stored as zero), out[2] = entries, then (bi, bj, kbeg, kend, slice) per entry (k in units of 16), as many entries as fit `cap` int64
 * values.  Returns 0, or ZIGP_EARG for an unknown rule, nb <= 0, out == NULL or cap < 3. */
int zigp_test_sk_list(int32_t rule, int32_t nb, int64_t cap, int64_t* out);
/* The gradient step of the larger fused grids (<= 16 x <= 112 points) sends its rows through in ranges of `tiles` 16-point tiles
 * (default 1024 = 16 384 rows: the per-point operand records of a range stay within 128 MB).  Results do not depend on it, bit for bit;
 * the tests lower it to run many ranges on small inputs. */
int zigp_set_kron_range_tiles(zigp_ctx* ctx, int32_t tiles);
/* C (m,n) = op(A) * op(B) with the fp64 MFMA GEMM core; transA/transB as BLAS; all dims padded internally. */
int zigp_test_gemm(zigp_ctx* ctx, int32_t transA, int32_t transB, int64_t m, int64_t n, int64_t k,
                   const double* A, const double* B, double* C);
/* L = chol(A) (lower), W = L^-1, A is (n,n) SPD; either output may be NULL.  split_k != 0: the blocked chain's products run as k slices +
 * an ordered reduction, as in the M x M forward of zigp_elbo (0: one workgroup per tile, as in the Kronecker panel path). */
int zigp_test_potrf_trtri(zigp_ctx* ctx, int64_t n, const double* A, double* L, double* W, int32_t split_k);
/* The same chain, tapped: ONE job of size n (1 .. 4096; padded to Mp = n rounded up to 128, nb = Mp / 128 block columns) through
 * potrf_trtri_jobs itself (csrc/zigp_host.h) -- the launches of zigp_test_potrf_trtri, none more, none fewer.  L, W, T: the WHOLE padded
 * [Mp][Mp] images as the chain leaves them (L, W: identity in the padding, exact zero above the diagonal; T, the scratch of the inverse:
 * ZIGP_STAGE_SENTINEL_BYTE wherever no launch wrote).  snap: [snap_cap][Mp][Mp] images, one stream-ordered device-to-device copy right
 * behind each launch, in launch order, downloaded after the call's one synchronisation: per block column j the diagonal kernel (two images:
 * L, then W), the panel product (L) and the trailing update (L) -- the last two only for j < nb - 1 -- then per doubling distance
 * b = 1, 2, 4 .. < nb the products tri1 (T) and tri2 (W).  The image behind one launch is the "before" image of the next (the panel product
 * runs in place).  snap_cap >= launches + nb, with launches = nb + 2 (nb - 1) + 2 ceil(log2 nb).
 * facts: ZIGP_PSF_REC header slots, then ZIGP_PSF_PER slots per launch: kind (ZIGP_PSL_*), j or b, output tiles, split-K slices S (0: one
 * workgroup per tile, split_k = 0), npan of a diagonal launch (32-row panels it factors; the rest of the block is identity), index of the
 * launch's first image (-1 without snap).  facts_cap >= ZIGP_PSF_REC + ZIGP_PSF_PER * launches.
 * A failed factorisation returns ZIGP_ENOTPD with zigp_last_info = the 1-based pivot (also facts[ZIGP_PSF_INFO]); L, W, T, snap and facts
 * are filled all the same (the failing diagonal kernel writes nothing, the launches behind it run on what is there).  Any out pointer may
 * be NULL.  ZIGP_EARG (context still usable): n outside 1 .. 4096, A == NULL, a capacity too small. */
enum { ZIGP_PSL_DIAG = 0, ZIGP_PSL_PANEL = 1, ZIGP_PSL_TRAIL = 2, ZIGP_PSL_TRI1 = 3, ZIGP_PSL_TRI2 = 4 };
enum { ZIGP_PSF_MP = 0, ZIGP_PSF_NB, ZIGP_PSF_LAUNCHES, ZIGP_PSF_IMAGES, ZIGP_PSF_INFO, ZIGP_PSF_REC = 8, ZIGP_PSF_PER = 6 };
typedef struct zigp_stage_potrf {
  int64_t n;
  int32_t split_k, reserved;
  const double* A;        /* (n,n) symmetric; the lower triangle is read */
  double *L, *W, *T;      /* out [Mp][Mp] */
  double* snap;           /* out [snap_cap][Mp][Mp] */
  int64_t snap_cap;
  int64_t* facts;         /* out [facts_cap] */
  int64_t facts_cap;
} zigp_stage_potrf;
int zigp_test_potrf_stages(zigp_ctx* ctx, const zigp_stage_potrf* a);

/* The chunk loop's cross-covariance kernel on its own: K (M,N) row-major = var * exp(-0.5 |(z_m - x_n) / ell|^2) as k_kuf_build writes a
 * Kuf panel (kern.K(X, Xnew), onofftf/main.py:266; its exponential is hand-written, see csrc/zigp_kernels.h).  X (N,D), Z (M,D), ell (D). */
int zigp_test_kuf(zigp_ctx* ctx, int64_t N, int32_t M, int32_t D, const double* X, const double* Z, const double* ell, double var, double* K);

/* ---- stage diagnostics: ONE chunk's stage of the dense chunk loop on caller-supplied operands, through the functions the loop itself
 * runs (chunk_plan -> upload_plan -> chunk_forward, the point-wise launch, latent_chunk_kgrad, latent_chunk_syrk + the plane reduction of
 * the M x M reverse stage).  Host arrays in, host arrays out; every call synchronises and leaves the context usable for zigp_elbo. ---- */
/* Device buffers the diagnostics fill before a launch hold this byte in every position (the double ZIGP_STAGE_SENTINEL_BYTE x 8 is
 * 1.38e306): an output element that still holds it was not written. */
#define ZIGP_STAGE_SENTINEL_BYTE 0x7f
typedef struct zigp_stage_latent {
  int32_t M, reserved;
  const double* W;    /* (M,M) lower triangular; padded to Mp with the identity, as the factorisation leaves it; W^T by k_transpose */
  const double* v;    /* (M)   weights of the fused sum v A1 (the mean) */
  const double* s2;   /* (M)   weights of sum s^2 A2^2 (value mode) */
  const double* K;    /* (M,Nc) Kuf panel; rows >= M are zero on the device */
  const double* Rt;   /* (M,M) gradient mode: what the J' launch reads as its factor, (Q W^T)^T; padded with -I (Q = -I where s^2 = 0) */
  double* A1;         /* out (M,Nc) */
  double* Jp;         /* out (M,Nc), gradient mode */
  double* part;       /* out [3][Mp/32][Nc]: the RAW partial-row planes; rows nothing wrote hold the sentinel */
} zigp_stage_latent;
/* Forward products of one chunk of Nc rows (a multiple of 1024) for both latents: A1 and the A2 sums (need_grad = 0) or A1 and J'
 * (need_grad = 1).  only = -1: both latents as the loop launches them; 0 / 1: the plan of the pair, that latent's lists alone (the other
 * latent's operands may then be NULL).  facts[12] = {paired, tail units f, tail units g, Mp_f, Mp_g, allocated partial rows per plane
 * f, g, then the counts the point-wise stage is told: np1_f, np2_f, np1_g, np2_g, 0}. */
int zigp_test_chunk_forward(zigp_ctx* ctx, int64_t Nc, int32_t need_grad, int32_t only, const zigp_stage_latent* lat /*[2]*/, int64_t* facts /*[12]*/);

/* What the M x M forward of a call leaves, downloaded: out_f / out_g [ZIGP_FWD_OUTS], indexed by ZIGP_FWD_*, any of them NULL.  Runs the
 * upload and the two factorisation chains of the context's parametrisation as zigp_elbo does: unwhitened, or whitened with a diagonal q_sqrt
 * (zigp_set_whiten); a full-covariance context is refused (zigp_test_q_full_forward has that stage).  An output the mode, or need_grad = 0,
 * does not produce is left untouched. */
enum {
  ZIGP_FWD_W = 0,      /* (M,M) W = L^-1 */
  ZIGP_FWD_V = 1,      /* (M)   v = W u                              unwhitened */
  ZIGP_FWD_ALPHA = 2,  /* (M)   alpha = W^T v;  whitened: W^T u (need_grad) */
  ZIGP_FWD_RT = 3,     /* (M,M) Rt = W Qt = (Q W^T)^T                unwhitened, need_grad */
  ZIGP_FWD_DKINV = 4,  /* (M)   diag(Kuu^-1) = column sums of W^2    unwhitened */
  ZIGP_FWD_KL = 5,     /* (1)   the latent's KL */
  ZIGP_FWD_P = 6,      /* (M,M) P = W^T W                            unwhitened, need_grad */
  ZIGP_FWD_QT = 7,     /* (M,M) Qt = diag(s^2) P - I                 unwhitened, need_grad */
  ZIGP_FWD_WP = 8,     /* (M,M) W diag(s^2);  whitened: D W = diag(s^2 - 1) W      need_grad */
  ZIGP_FWD_WT = 9,     /* (M,M) W^T */
  ZIGP_FWD_WH = 10,    /* (3,M) whitened: the block k_kl_white leaves: s^2 - 1, u, 1 */
  ZIGP_FWD_L = 11,     /* (M,M) L = chol(Kuu) */
  ZIGP_FWD_KUU = 12,   /* (M,M) Kuu + jitter I as k_kuu_setup writes it */
  ZIGP_FWD_OUTS = 13
};
int zigp_test_latents_forward(zigp_ctx* ctx, const zigp_params* p, double jitter, int32_t need_grad, double* const* out_f, double* const* out_g);

typedef struct zigp_stage_pointwise {
  int32_t mode;       /* 0 value-only ELBO, 1 gradient step, 2 predict */
  int32_t repeat;     /* launches (>= 1): acc keeps accumulating */
  int32_t np_f, np1_f, np2_f, np_g, np1_g, np2_g;   /* allocated rows per plane, rows of planes 0 / 1 and of plane 2 to add */
  int32_t D, mean_on;
  const double* part_f;   /* [3][np_f][Nc] */
  const double* part_g;   /* [3][np_g][Nc] */
  const double* Y;        /* [Nrows] (NULL: predict) */
  const double* X;        /* [Nrows][D] */
  int64_t Nrows, n0, row_end, Nc;
  double var_f, var_g, noise, g_offset, scale;
  double mean_a[8], mean_b;
  double *gm_f, *gv_f, *gm_g, *gv_g;   /* out [Nc] each (gradient step) */
  double* acc;            /* in / out [Nc/64][13]: the per-block accumulators */
  double* out9;           /* out [9][row_end] (predict) */
} zigp_stage_pointwise;
int zigp_test_pointwise(zigp_ctx* ctx, const zigp_stage_pointwise* a);

/* Kuf cotangent reductions of one chunk: krow [4][M][2+2D] (the KG_SPLIT slabs; in: initial values, out: accumulated).  X (Nrows,D),
 * Z (M,D), Jp / K (M,Nc), alpha (M), gm / gv (Nc).  exact = 0 / 1 forces the centred / the per-row form, -1 takes the host's rule (needs
 * ell); centre = NULL: the mean inducing input, as the host computes it. */
int zigp_test_kgrad(zigp_ctx* ctx, int32_t M, int32_t D, int64_t Nc, int64_t Nrows, int64_t n0, const double* Jp, const double* K,
                    const double* alpha, const double* gm, const double* gv, const double* X, const double* Z, const double* ell,
                    const double* centre, int32_t exact, double* krow);

/* The counterpart of zigp_test_kuf for a kernel kind (ZIGP_KERN_*, include/zigp.h): the Kuf panel as a call with that kind on the
 * latent builds it (kernels.Matern32.K / Matern52.K of GPflow 0.4.0 in place of RBF.K at onofftf/main.py:266) and, when Kd != NULL,
 * the derivative panel K' = -dk / d(r2 / 2) a gradient step writes in the same launch (K' = K for ZIGP_KERN_RBF, copied).  K and Kd
 * are (Mp16, N) row-major with Mp16 = M rounded up to 16: the rows m >= M of the last 16-row group are returned too (zeros).
 * D <= 8 for the Matern kinds. */
int zigp_test_kuf_kind(zigp_ctx* ctx, int32_t kind, int64_t N, int32_t M, int32_t D, const double* X, const double* Z, const double* ell,
                       double var, double* K, double* Kd);
/* The counterpart of zigp_test_kgrad for a kernel kind: the Kuf cotangent reductions of one chunk as a gradient step with that kind on
 * the latent launches them (the reverse of kernels.Matern32.K / Matern52.K; of KernSE.K, onofftf/main.py:41-57, for ZIGP_KERN_RBF,
 * where Kd is not read and the per-row form of k_kgrad runs).  Kd (M,Nc): the derivative panel; the
 * 2 D moment columns of krow are taken with F Kd, columns 0 and 1 + 2 D with K.  Other arguments as zigp_test_kgrad. */
int zigp_test_kgrad_kind(zigp_ctx* ctx, int32_t kind, int32_t M, int32_t D, int64_t Nc, int64_t Nrows, int64_t n0, const double* Jp,
                         const double* K, const double* Kd, const double* alpha, const double* gm, const double* gv, const double* X,
                         const double* Z, double* krow);

/* Rank-N update C1 = sum_chunks A1_i diag(gv_i) A1_i^T: the chunks' updates one after the other onto zeroed split-K planes, then the
 * plane reduction.  A1[i] (M,Nc[i]), gv[i] (Nc[i]), Nc[i] multiples of 1024.  C1 (M,M) symmetric; plan[2] = {So, Sd}. */
int zigp_test_rank_update(zigp_ctx* ctx, int32_t M, int32_t nchunks, const int64_t* Nc, const double* const* A1, const double* const* gv,
                          double* C1, int64_t* plan /*[2]*/);

/* ---- whitened parametrisation (zigp_set_whiten): the stages that differ, through chunk_forward_white and the point-wise launch of a
 * whitened call.  The structs are the ones above, read as follows. ---- */
/* Forward products of one whitened chunk.  zigp_stage_latent: W as above; v = the weights of the mean sum (u); s2 = the weights of the
 * variance sum (s^2 - 1; any sign); K as above; Rt (M,M) = what the J' launch reads as its factor, the image D W (row k of W scaled by
 * s_k^2 - 1), zero padded, so that J' = Rt^T A.  need_grad = 0: the launch A = W K alone, with the non-storing epilogue -- A1 is not
 * written and may be NULL; need_grad = 1: A (stored to A1) and J' = (W^T D) A (stored to Jp).  part [3][Mp/32][Nc]: plane 0 = partial
 * rows of sum_m v_m A_mn, plane 2 = of sum_m s2_m A_mn^2, plane 1 is not written (sentinel).  only and facts as zigp_test_chunk_forward. */
int zigp_test_chunk_forward_white(zigp_ctx* ctx, int64_t Nc, int32_t need_grad, int32_t only, const zigp_stage_latent* lat /*[2]*/, int64_t* facts /*[12]*/);
/* The point-wise stage as a whitened call launches it: in every mode mean = sum of plane 0 (np1 rows), var = var_* + sum of plane 2 (np2
 * rows); plane 1 is not read.  Arguments as zigp_test_pointwise. */
int zigp_test_pointwise_white(zigp_ctx* ctx, const zigp_stage_pointwise* a);
/* One launch (a->repeat launches) of the head's point-wise kernel (zigp_head_elbo / zigp_head_predict, include/zigp.h) on caller-supplied
 * partial planes of f: lik = ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI; white = 0 reads the planes as zigp_test_pointwise does (mode 0 and 2:
 * var = var_f - plane 1 + plane 2; mode 1: var_f + plane 2), white = 1 as zigp_test_pointwise_white (var_f + plane 2 in every mode).
 * part_g, np*_g, var_g and g_offset are not read (part_g may be NULL); gm_g / gv_g come back as the zeros the kernel writes; out9 is the
 * head's block, [4][row_end]: fmean, fvar, pfmean, pfvar; acc slot 3 is left as it was. */
int zigp_test_pointwise_head(zigp_ctx* ctx, int32_t lik, int32_t white, const zigp_stage_pointwise* a);

/* ---- full-covariance q(u) (zigp_set_q_full): the M x M stage of one latent.  The chunk loop of such a call runs the unwhitened
 * launches (zigp_test_chunk_forward with v = u, s2 = 1, W -> Lq for the second product, Rt = (T - I) W), so only this stage is new. ---- */
/* Forward: W (M,M) lower triangular, Lq (M,M) as the caller of zigp_elbo passes it (the strict upper triangle is ignored, the diagonal
 * must be non-zero), u (M).  Returns, each (M,M) row-major or NULL: TmI = tril(Lq) tril(Lq)^T - I; Rt = TmI W, the image the J' launch
 * reads (J' = Rt^T A); and *kl = 0.5 (sum u^2 + sum_{i>=j} Lq_ij^2 - M - sum_i log Lq_ii^2). */
int zigp_test_q_full_forward(zigp_ctx* ctx, int32_t M, const double* W, const double* Lq, const double* u, double* TmI, double* Rt, double* kl);
/* Backward: dLq (M,M) = tril(2 C1 Lq) - [include_kl] (tril(Lq) - diag(1 / Lq_ii)) for a symmetric C1 (M,M); strict upper triangle 0. */
int zigp_test_q_full_dlq(zigp_ctx* ctx, int32_t M, const double* C1, const double* Lq, int32_t include_kl, double* dLq);

/* ---- the M x M reverse stage of ONE latent on caller-supplied operands, through latent_mxm_backward itself
 * (the chain of split-K products, their finishers and the element-wise / reduction kernels between them, then k_kuu_grad[_wide]).  The
 * call's accumulators are sized and zeroed by the step's own path (dense_prepare_buffers) before the operands go in: C1 as the rank-update
 * planes (tril(C1) in plane 0, zeros in the others, so that k_sym_from_planes runs as in a step), krow as given.  The derived images come
 * from the forward stage's kernels: W diag(s^2) (k_colscale), D W (k_kl_white + k_rowscale), or the staged factor, T - I and R^T
 * (latent_qfull_stage / _factors).  The M x M scratch buffers hold the stage sentinel before the first launch. ---- */
/* Taps: one (M,M) copy taken right after the launch that produces the value and before its buffer is reused. */
enum {
  ZIGP_MXM_TAP_C1 = 0,   /* C1 after the plane sum (k_sym_from_planes) */
  ZIGP_MXM_TAP_Y = 1,    /* unwhitened: Y = C1 W ("y");  full covariance: Y = C1 Lq ("y", latent_qfull_dlq) */
  ZIGP_MXM_TAP_T = 2,    /* T = (W diag(s^2)) W^T ("tt") */
  ZIGP_MXM_TAP_U = 3,    /* U = T C1 ("full") */
  ZIGP_MXM_TAP_V = 4,    /* V = U + U^T - C1 (k_uut_minus) */
  ZIGP_MXM_TAP_R = 5,    /* R: W^T V, (W^T D) C1 ("r") or (W^T (T - I)) C1 ("rfull"); lower tiles */
  ZIGP_MXM_TAP_DL = 6,   /* dL (k_dl_assemble) */
  ZIGP_MXM_TAP_Q = 7,    /* Q = Phi(L^T dL) ("r" + SK_PHI) */
  ZIGP_MXM_TAP_QW = 8,   /* Q W ("t"); lower tiles */
  ZIGP_MXM_TAP_S = 9,    /* S = W^T (Q W) ("s") */
  ZIGP_MXM_TAP_P = 10,   /* P = W^T W, when the stage forms it (P == NULL, with_kl) */
  ZIGP_MXM_TAP_PSP = 11, /* P diag(s^2) P ("full"), with_kl, unwhitened */
  ZIGP_MXM_TAPS = 12
};
typedef struct zigp_stage_mxm {
  int32_t M, D;
  int32_t mode;        /* 0 unwhitened, 1 whitened with a diagonal q_sqrt, 2 whitened with a full-covariance q_sqrt */
  int32_t with_data, with_kl;   /* as the step passes them: has rows / include_kl */
  int32_t reserved;
  double jitter;
  double pad;          /* what the padding (index >= M) of Z, Kuu, s and plane 0 of C1 holds on the device; a step leaves 0 there */
  const double* W;     /* (M,M) lower triangular; padded to Mp with the identity */
  const double* L;     /* (M,M) lower triangular; padded to Mp with the identity */
  const double* Kuu;   /* (M,M) */
  const double* Z;     /* (M,D) */
  const double* s;     /* modes 0, 1: (M), non-zero;  mode 2: Lq (M,M), non-zero diagonal (the strict upper triangle is ignored) */
  const double* u;     /* (M) or NULL (zeros): modes 1, 2, for the whitened vectors (the stage itself does not read it) */
  const double* v;     /* (M) mode 0: W u */
  const double* alpha; /* (M): W^T v (mode 0), W^T u (modes 1, 2) */
  const double* P;     /* (M,M) mode 0: W^T W as the forward stage leaves it, or NULL: P_ready is false and the stage forms it */
  const double* C1;    /* (M,M) symmetric (with_data) */
  double* krow;        /* in / out [4][Mp][2+2D]: the WHOLE device buffer, padded rows included.  In: initial values; sum_slabs of column
                          1 + 2D is K gm.  Out: what the stage left (it adds to slab 0, rows < M) */
  double* a1gm;        /* out (M): W (K gm) */
  double* du;          /* out (M): W^T a1gm (mode 0; stays zero otherwise) */
  double* dsq;         /* out (M): diag(W^T C1 W) (mode 0), diag(C1) (mode 1); as zeroed in mode 2 */
  double* dLq;         /* out (M,M), mode 2 */
  double* G;           /* out (M,M): what k_kuu_grad reads */
  double* tap[ZIGP_MXM_TAPS];   /* out (M,M) each or NULL; a tap its mode does not pass is left untouched */
} zigp_stage_mxm;
/* Any out pointer may be NULL.  Returns ZIGP_EARG (context still usable) for M <= 0, D outside 1 .. ZIGP_MAX_D, a mode outside 0 .. 2, a
 * missing operand of the mode, or a zero on the diagonal of s / Lq. */
int zigp_test_mxm_backward(zigp_ctx* ctx, const zigp_stage_mxm* a);

/* ---- the call's result vector from caller-supplied accumulators, through dense_pack (k_dense_pack, and k_pack_square for mode 2) ---- */
typedef struct zigp_stage_pack_latent {
  int32_t M, reserved;
  const double* krow;     /* [4][M][2+2D]: all KG_SPLIT slabs */
  const double* du;       /* (M) mode 0: du;  modes 1, 2: W (K gm), what a whitened call packs as du's data part */
  const double* dsq;      /* (M) modes 0, 1 */
  const double* s;        /* (M) modes 0, 1, non-zero */
  const double* dLq;      /* (M,M) mode 2 */
  const double* kl_vec1;  /* (M) dKL/du: alpha (mode 0), u (modes 1, 2) */
  const double* kl_vec2;  /* (M) c of dKL/ds = -1/s + c s: diag(Kuu^-1) (mode 0), ones (mode 1); mode 2: not used, may be NULL */
  const double* ell;      /* (D) */
  double var, kl;         /* kernel variance; the latent's KL value */
} zigp_stage_pack_latent;
typedef struct zigp_stage_pack {
  int32_t D, mode;        /* mode as zigp_stage_mxm */
  int32_t need_grad, include_kl, mean_on, pw_blocks;
  const double* pw;       /* [pw_blocks][13]: the point-wise stage's per-block accumulators */
  zigp_stage_pack_latent lat[2];
  double* out;            /* [n_out] the packed vector: 16 header doubles, then per latent dZ (M,D), du (M), ds (M; mode 2: dLq (M,M)), dell (D) */
  int64_t n_out;          /* must be what the flags imply (16 without need_grad) */
} zigp_stage_pack;
int zigp_test_dense_pack(zigp_ctx* ctx, const zigp_stage_pack* a);

/* ---- Kronecker path: ONE launch of a point-wise or per-point panel kernel (csrc/zigp_kron.hip) on caller-supplied operands, with the grid
 * its production callers use.  Host arrays in, host arrays out; every call synchronises and leaves the context usable. ---- */
/* The point-wise launch of a Kronecker call: k_kron_pointwise<PREDICT> (lik = ZIGP_LIK_ONOFF), k_kron_head_pointwise<PREDICT, false>, or, with
 * dev_hyp = 1 on a head, k_kron_head_pointwise<false, true> (modes 0 and 1 only: no call launches the heads' predict kernel on the device
 * block).  Grid Nc / 256 blocks of 256 points.  dev_hyp = 0: Knn = var0 var1 per latent, the noise and f_offset go in by value, as the
 * panel path passes them.  dev_hyp = 1: they are read from a device hyperparameter block filled by the host code of the fused path (the
 * factor records' variances, the noise; f_offset in the slot a device fit step keeps f_mu in -- the OnOff kernel takes f_offset by value in
 * either case), and the by-value fields are zero. */
typedef struct zigp_stage_kron_pointwise {
  int32_t lik;            /* ZIGP_LIK_ONOFF / ZIGP_LIK_GAUSSIAN / ZIGP_LIK_BERNOULLI */
  int32_t mode;           /* 0 value-only ELBO (the launch with gm_f == NULL), 1 gradient step, 2 predict */
  int32_t dev_hyp;        /* 0 / 1 */
  int32_t sentinel_out;   /* 1: every output buffer holds ZIGP_STAGE_SENTINEL_BYTE before the launch (0: zeros) */
  int64_t N, Nc;          /* valid points; points launched: a multiple of 256, >= N */
  int64_t ld_out;         /* predict: leading dimension of out, >= N (0: N, as the real calls) */
  const double* part_f;   /* [4][Nc]: q0, q1, mean, st */
  const double* part_g;   /* [4][Nc] (OnOff; the heads do not read it, may be NULL) */
  const double* Y;        /* [N] (NULL: predict) */
  double var0f, var1f, var0g, var1g, noise, g_offset, f_offset, scale;
  double *gm_f, *gv_f, *dq0_f, *dq1_f, *gm_g, *gv_g, *dq0_g, *dq1_g;   /* out [Nc] each, modes 0 and 1, any of them NULL; the buffers as the
                             launch left them -- mode 0 writes none of them, a head none of the g ones */
  double* acc;            /* out [Nc / 256][5], modes 0 and 1: ve, d noise, sum gv_f, sum gv_g, sum gm_f per block */
  double* out;            /* out [9 or 4][ld_out], predict */
} zigp_stage_kron_pointwise;
int zigp_test_kron_pointwise(zigp_ctx* ctx, const zigp_stage_kron_pointwise* a);

/* The panel path's per-point kernels, one launch each with the grid of latent_forward_panels / latent_backward.  Nc: a multiple of 256; panels
 * are row-major with Nc columns.  Output buffers hold the stage sentinel before the launch. */
/* k_kron_kbuild: K (Mq, Nc), Mq = M rounded up to 128, = var exp(-0.5 |(z_m - x_n[col0 : col0 + D]) / ell|^2); X (N, ldx), Z (M, D), ell (D).
 * The whole padded panel is returned: rows m >= M (zeros) and columns n >= N (the kernel at x = 0). */
int zigp_test_kron_kbuild(zigp_ctx* ctx, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, int32_t M, int32_t D, const double* X, const double* Z,
                          const double* ell, double var, double* K);
/* k_kron_colsum: part [4][Nc] = column sums of K0.A0, K1.A1, K0.B1 and A0sq.C1; K0, A0, B1, A0sq, C1 (M0, Nc), K1, A1 (M1, Nc). */
int zigp_test_kron_colsum(zigp_ctx* ctx, int32_t M0, int32_t M1, int64_t Nc, const double* K0, const double* A0, const double* K1, const double* A1,
                          const double* B1, const double* A0sq, const double* C1, double* part);
/* k_kron_da: dA = 2 A gv C, E = dq K + dA over a panel of M rows (padded with zero rows to a multiple of 128 on the device, as the panels
 * of a step are); A, C, K, dA, E (M, Nc), gv, dq (Nc). */
int zigp_test_kron_da(zigp_ctx* ctx, int32_t M, int64_t Nc, const double* A, const double* C, const double* K, const double* gv, const double* dq,
                      double* dA, double* E);
/* k_kron_kgrad: krow (M, 2 + 2D), in: initial values, out: with the row's sums over the columns n < N added to columns 0 .. 2D (the last
 * column is not touched); B, A, PdA, K (M, Nc), gm, dq (Nc), X (N, ldx), Z (M, D). */
int zigp_test_kron_kgrad(zigp_ctx* ctx, int32_t M, int32_t D, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, const double* B, const double* A,
                         const double* PdA, const double* K, const double* gm, const double* dq, const double* X, const double* Z, double* krow);

/* The factor panel of any ZIGP_KERN_* kind, through the launch latent_forward_panels makes for that kind: K and (Kd != NULL: a gradient step)
 * the derivative panel K' = -dk / d(r2 / 2), both (Mq, Nc) as zigp_test_kron_kbuild returns K.  ZIGP_KERN_RBF runs k_kron_kbuild (K' = K);
 * a Matern kind k_kron_kbuild_matern<KIND, Kd != NULL>. */
int zigp_test_kron_kbuild_kind(zigp_ctx* ctx, int32_t kind, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, int32_t M, int32_t D, const double* X,
                               const double* Z, const double* ell, double var, double* K, double* Kd);
/* The factor cotangent of any kind: zigp_test_kron_kgrad's arguments plus Kd (M, Nc).  ZIGP_KERN_RBF runs k_kron_kgrad (Kd is not read); a Matern
 * kind k_kron_kgrad_matern: column 0 takes dK K, the 2 D moment columns dK K'. */
int zigp_test_kron_kgrad_kind(zigp_ctx* ctx, int32_t kind, int32_t M, int32_t D, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, const double* B,
                              const double* A, const double* PdA, const double* K, const double* Kd, const double* gm, const double* dq,
                              const double* X, const double* Z, double* krow);

/* ---- Fused Kronecker path (csrc/zigp_kronf.hip, zigp_kronl.h): ONE ordinary value-and-gradient step through the host code of
 * zigp_kron_elbo / zigp_kron_head_elbo itself -- same plan, launches, grids and device buffers, zigp_set_kron_range_tiles honoured -- with
 * device buffers snapshot around it.  Every tap is optional (NULL: not taken); a tap is a stream-ordered device-to-device copy enqueued
 * right after the launch that produces the value, downloaded when the step has finished, so a later kernel that reuses the buffer cannot
 * matter.  The caller sizes the host arrays: Mq_p = M_p rounded up to 16 (the latent's OWN padded sizes), nb_p = Mq_p / 16,
 * Npad = max(1024, N rounded up to 1024); the capacity (nb0c, nb1c) is (2, 2) when every M_p <= 32, else (1, 7) (M0 <= 16, M1 <= 112).
 * Returns ZIGP_EARG for a grid beyond the fused kernels, or one forced onto the panel path (zigp_set_kron_panels). ---- */
typedef struct zigp_kronf_tap_factor {   /* after k_kf_factor */
  double* K;      /* [128][128] K_p + jitter I; only the leading [R][R] part is written, R = M_p rounded up to 32, identity-padded beyond M_p */
  double* P;      /* [Mq][Mq] row-major K_p^-1, zero rows / columns >= M_p */
  double* PF;     /* [Mq * Mq] raw: P in A-fragment order, F[(rb * (Mq / 4) + ks) * 64 + lane] = P(16 rb + lane % 16, 4 ks + lane / 16) */
  double* dvec;   /* [Mq + 1]: diag(P), then logdet K_p */
  double* Zs;     /* [Mq][D_p] inducing inputs times 1 / ell, zero rows >= M_p */
  double* zc;     /* [D_p] centre of the moment sums: the mid-range of the inducing inputs */
} zigp_kronf_tap_factor;
typedef struct zigp_kronf_tap_latent {
  zigp_kronf_tap_factor fac[2];
  double *U, *S2, *T0, *T1, *Al;       /* after k_kf_latent / k_kfl_latent: [Mq0][Mq1] row-major each, zero padded: u, s^2, U P1, P0 U, P0 U P1 */
  double *AlF, *S2F, *AlTF, *S2TF;     /* [Mq0 * Mq1] raw fragment images of Al, S2 ([nb0][Mq1 / 4][64]) and of their transposes ([nb1][Mq0 / 4][64]) */
  double* part;    /* after the forward kernel: [4][Npad] = q0, q1, mean, S-term */
  double* cot;     /* after the point-wise kernel (before any injection): [4][Npad] = gm, gv, dq0, dq1 */
  double* work;    /* after k_kf_reduce: the latent's whole work block, capacity rows and columns included.  With R_p = 16 nb_pc and
                      ldw = max(R0, R1):  dAl [R0][ldw] | dS2 [R0][ldw] | dP0 [R0][ldw] | dP1 [R1][ldw] | Kr0 [R0][16] | Kr1 [R1][16]
                      (sums over points, unsymmetrised dP_p = sum E_p K_p^T; Kr_p[m][j] = sum_n t_p[m, n] psi_j(x_n), psi = {1, x - zc, (x - zc)^2}) */
  const double* inject;   /* in, optional: [4][N] copied over gm, gv, dq0, dq1 between the point-wise launch and the backward launch; rows >= N keep
                             what the point-wise kernel wrote */
  /* ---- the finish stage (k_kf_finish; larger grids k_kfl_finish<1..3>; Matern factors: k_kf_kd_prepare / k_kf_krow_merge, k_kfl_krow_kinds).
   * Capacity rows R_p = 16 nb_pc (32, 32 or 16, 112), ldw = max(R0, R1), W = 2 + 2 * 8 = 18 doubles per capacity row of a krow region.
   * UNWRITTEN PARTS.  Every tap below is taken at the capacity size of its region.  When one of them is asked for, the hook fills the region
   * with ZIGP_STAGE_SENTINEL_BYTE before the step's first launch that could write it -- the latents' result blocks (klv, krow, gu, gs,
   * krow_first) at the start of the step, the scratch of the second small-grid run (Kd, krow2) before k_kf_kd_prepare, the G regions before
   * k_kfl_finish<1> -- so an element the kernels never write comes back as the sentinel, and a kernel that wrote past its compact part shows.
   * Nothing reads those elements (the step returns the bits of an ordinary call).  In a data-parallel context (zigp_comm_init) the step itself
   * clears the result blocks, and their unwritten elements are +0 instead.  Padding the kernels DO write is exact zero: named per tap. */
  double* klv;            /* after k_kf_latent / k_kfl_latent: [8] = sum U.Alpha, sum log s^2, sum d0 d1 s^2, logdet K0, logdet K1; [5..7] unwritten */
  double* krow[2];        /* after the LAST launch of the stage: the region [R_p * W] of the result block.  The kernels write it COMPACTLY,
                             [M_p][2 + 2 D_p] from its start (column 0: d var numerator, 1 .. D: d Z, D + 1 .. 2 D: d ell numerators, 1 + 2 D: exact 0);
                             everything behind M_p (2 + 2 D_p) is unwritten */
  double *gu, *gs;        /* after the last launch: [R0 * R1] regions of the result block, written compactly as [M0 * M1]; the rest is unwritten */
  double* krow_first[2];  /* a step with a Matern factor: the krow regions (as `krow`) after the first k_kf_finish, before k_kf_krow_merge overwrites
                             columns 1 .. 2 D of a Matern factor; larger grids: after k_kfl_finish<3>, before k_kfl_krow_kinds rewrites the rows of a
                             Matern factor.  Not taken (the host array is left alone) by a step whose factors are all RBF */
  double* Kd[2];          /* small grids with a Matern factor, after k_kf_kd_prepare: the [32][128] image K'_p(Z_p, Z_p) = -dk / d(r2 / 2) the second
                             k_kf_finish reads in place of K_p.  The kernel writes the leading [M_p][M_p] entries of a Matern factor (row stride 128);
                             everything else -- the whole image of an RBF factor included -- is unwritten */
  double* work2;          /* same step, after k_kf_kd_prepare: the copy of the work block (layout of `work`, capacity (2, 2): 4 * 32 * 32 + 2 * 32 * 16
                             doubles) with column 0 of the moment block of every Matern factor replaced by its column 15; every element is written */
  double* krow2[2];       /* same step, after the second k_kf_finish (on Kd / work2): [32 * W] regions written compactly as `krow`; the rest is unwritten */
  double* G[2];           /* larger grids, after k_kfl_finish<3> (before k_kfl_krow_kinds): the [ldw][ldw] region of the factor's scratch set the
                             stage leaves its G rows in (row stride ldw = 112).  Factor 0: rows 0 .. Mq0 - 1, columns < Mq0 hold
                             G = -P sym(dP') P - coef P itself (compensated, rounded once), rows 16 .. 16 + Mq0 - 1 the low words of Q2 = X P that
                             stage 2 left there.  Factor 1: rows and columns < Mq1 hold the plain product P Q2 = P X P; the kernels form
                             G = -that - coef P on the fly when they read it.  Rows / columns M_p .. Mq_p - 1 of G and P Q2 are written: exact
                             (signed) zeros.  Everything else is unwritten */
} zigp_kronf_tap_latent;
/* facts[] of zigp_test_kron_fused_step */
enum { ZIGP_KFF_LARGE = 0,     /* 1: the larger-grid kernels (k_kfl_*), 0: the small-grid ones (k_kf_*) */
       ZIGP_KFF_LARGE_EXACT,   /* 1: the larger-grid instantiation with compile-time block counts */
       ZIGP_KFF_NB0C, ZIGP_KFF_NB1C,                                      /* capacity block counts */
       ZIGP_KFF_NB0_F, ZIGP_KFF_NB1_F, ZIGP_KFF_NB0_G, ZIGP_KFF_NB1_G,    /* each latent's own block counts (a head: g = f) */
       ZIGP_KFF_NPAD, ZIGP_KFF_NTILES,
       ZIGP_KFF_TPW_FWD,       /* tiles per wave of the forward launch */
       ZIGP_KFF_TPW_BWD,       /* tiles per wave of the backward launch (larger grids: of its first row range) */
       ZIGP_KFF_NPARTS,        /* partial accumulators k_kf_reduce sums per latent */
       ZIGP_KFF_TPS,           /* larger grids: tiles per part of k_kfl_accum (0: small grids) */
       ZIGP_KFF_NRANGES,       /* larger grids: row ranges = backward + accumulate launch pairs (1: small grids) */
       ZIGP_KFF_RANGE_TILES,   /* larger grids: tiles per range (0: small grids) */
       ZIGP_KFF_ONE_LAUNCH,    /* 1: the point kernels took both latents (or the only one) in one launch */
       ZIGP_KFF_COUNT };
typedef struct zigp_stage_kron_fused {
  int32_t lik;                  /* ZIGP_LIK_ONOFF (two latents) or a head (the f fields of everything) */
  int32_t include_kl;
  const zigp_kron_params* p;
  const double *X, *Y;          /* host [N][D0 + D1], [N] */
  int64_t N;                    /* >= 1 */
  double jitter, scale, g_offset, f_mu;
  zigp_kronf_tap_latent lat[2];
  int64_t* facts;               /* out [ZIGP_KFF_COUNT], may be NULL */
  double *elbo_data, *kl;       /* the step's ordinary outputs (of the injected cotangents, when there are any) */
  zigp_kron_grads* grads;       /* required: the hook runs the gradient step */
  double* d_f_mu;
} zigp_stage_kron_fused;
int zigp_test_kron_fused_step(zigp_ctx* ctx, const zigp_stage_kron_fused* a);

/* ---- One ordinary value-and-gradient step of the GEMM-PANEL path (kron_run_panels, csrc/zigp_kron.hip: grids beyond the fused kernels, D = 8,
 * Matern factors without the opt-in, or zigp_set_kron_panels) through the production host code itself: the same launches, streams and
 * buffers.  A tap is a stream-ordered device-to-device copy enqueued right behind the producing launch, on that latent's stream, into a
 * buffer of its own, and downloaded after the step; a NULL tap is not taken.  The step returns the bits of an ordinary call (of the
 * injected cotangents, when there are any).  Sizes: Mq_p = M_p rounded up to 128, Nc = max(1024, N rounded up to 1024); M x M taps are the
 * whole padded [Mq][Mq] image (row stride Mq), grid taps [Mq0][Mq1] (row stride Mq1). ---- */
typedef struct zigp_kronp_tap_factor {
  double *K;        /* after the K_p launch: K_p + jitter I on [M][M], identity in the padding */
  double *L, *W;    /* after potrf_trtri: the Cholesky factor (lower triangle; taken before the backward pass reuses the buffer) and its inverse */
  double *P;        /* after P = W^T W: K_p^-1, identity in the padding */
  double *krow_n;   /* [Mq][2 + 2 D] after k_kron_kgrad (the sums over points), before the Kuu-gradient kernel adds to it */
  double *dP_red;   /* after the split-K reduction dP_p = sum_n E_p K_p^T */
  double *dP_acc;   /* after the EpiAccum product: + dAl T0^T (p = 0), + (P0 U)^T dAl (p = 1) */
  double *Q;        /* include_kl: the factor's G buffer after the KL product, Q0 = T0 U^T or Q1 = U^T (P0 U) */
  double *dP_comb;  /* after k_kron_dp_combine */
  double *T;        /* T = dP P */
  double *PdPP;     /* P T, in the buffer L held */
  double *G;        /* after k_kron_dk */
  double *krow;     /* [Mq][2 + 2 D] after the Kuu-gradient kernel */
} zigp_kronp_tap_factor;
typedef struct zigp_kronp_tap_latent {
  zigp_kronp_tap_factor f[2];
  double *U, *S2, *T0, *Al;   /* after latent_setup's uploads and products: T0 = U P1, Al = P0 T0; zeros in the padding */
  double *vec;                /* [Mq0 + Mq1]: diag(P0), diag(P1) */
  double *klv;                /* include_kl: [5] = sum U.Alpha, sum log s^2, sum d0 d1 s^2, logdet K0, logdet K1 */
  double *part;               /* [4][Nc] column sums after the forward panels */
  const double* inject;       /* in, optional: [4][N] copied over gm, gv, dq0, dq1 behind the point-wise launch; columns >= N keep what it wrote */
  double *cot;                /* [4][Nc]: gm, gv, dq0, dq1 as the backward pass reads them */
  int32_t planes_of;          /* which split-K reduction `planes` is taken from: 0 dP0, 1 dP1, 2 dAl, 3 dS2 */
  double *planes;             /* [S][nba 128][nbb 128] raw planes of that reduction, before k_sum_planes (S: facts) */
  double *dAl, *dS2;          /* after their reductions */
  double *T1_a, *dU;          /* T1 = dAl P1 ; dU = P0 T1 */
  double *T1_b;               /* T1 = P0 U (its second use) */
  double *gu, *gs;            /* [M0 M1], compact, after k_kron_us */
} zigp_kronp_tap_latent;
/* facts[] of zigp_test_kron_panel_step: ZIGP_KPF_NC, then per latent h at ZIGP_KPF_LAT + h * ZIGP_KPF_PER_LAT + ... */
enum { ZIGP_KPF_NC = 0, ZIGP_KPF_NK, ZIGP_KPF_LAT,
       ZIGP_KPF_MQ0 = 0, ZIGP_KPF_MQ1, ZIGP_KPF_NB0, ZIGP_KPF_NB1,
       ZIGP_KPF_S_DP0, ZIGP_KPF_S_DP1, ZIGP_KPF_S_DAL, ZIGP_KPF_S_DS2,      /* split-K slices of each reduction, in planes_of order */
       ZIGP_KPF_PER_LAT,
       ZIGP_KPF_COUNT = ZIGP_KPF_LAT + 2 * ZIGP_KPF_PER_LAT };
typedef struct zigp_stage_kron_panels {
  int32_t lik;                  /* ZIGP_LIK_ONOFF (two latents) or a head (the f fields of everything) */
  int32_t include_kl;
  const zigp_kron_params* p;
  const double *X, *Y;          /* host [N][D0 + D1], [N] */
  int64_t N;                    /* >= 1 */
  double jitter, scale, g_offset, f_mu;
  zigp_kronp_tap_latent lat[2];
  int64_t* facts;               /* out [ZIGP_KPF_COUNT], may be NULL */
  double *elbo_data, *kl;       /* the step's ordinary outputs */
  zigp_kron_grads* grads;       /* required: the hook runs the gradient step */
  double* d_f_mu;
} zigp_stage_kron_panels;
/* Refuses (ZIGP_EARG) a step that an ordinary call would run on the fused kernels, unless zigp_set_kron_panels is on. */
int zigp_test_kron_panel_step(zigp_ctx* ctx, const zigp_stage_kron_panels* a);

/* ---- The update kernels of the device fit loops, through the host loops themselves with the gradient step replaced by caller-supplied
 * results.  Nothing but the update / image kernels is launched; no rows and (Kronecker) no resident data set are needed.  Snapshots are
 * stream-ordered device-to-device copies behind the launches, downloaded after the loop's one synchronisation.  Both hooks return what the
 * loop returns (ZIGP_OK, or ZIGP_ENOTPD for an injected Cholesky status: the snapshots and records are filled in either case) and leave
 * the context usable. ---- */
/* k_fit_update<false> (lik = ZIGP_LIK_ONOFF, the 17 blocks of zigp_kron_fit_steps) or k_fit_update<true> (a head, the 10 blocks of
 * zigp_kron_head_fit_steps) through kf_fit_run: the production descriptor, grid, launches, lr_sq / lr_den, download and failure decoding.
 * Step i copies res + i * n_res into the result block in place of running the step.  Result block (doubles, offsets in facts): per latent h
 * at h * RES_SIZE: klv[5] at RES_KLV, krow of factor q at RES_KROW0 / RES_KROW1 written compactly as [M_q][2 + 2 D_q], gu / gs [M0 M1] at
 * RES_GU / RES_GS; then pws[8] at RES_PWS (data term, d noise, sum gv_f, sum gv_g, sum gm_f, -, -, ranks that count the KL) and at
 * RES_INFO four Cholesky status slots of 2 ints each (the first int of slot j is job j's pivot, 0 = fine).
 * res == NULL: only facts is filled (the layout query the caller sizes res, snap_img with).
 * Refused (ZIGP_EARG) like the fit calls: a grid beyond the fused kernels (a factor dimension above 7 included), zigp_set_kron_panels. */
enum { ZIGP_KFU_RES_KLV = 0, ZIGP_KFU_RES_KROW0, ZIGP_KFU_RES_KROW1, ZIGP_KFU_RES_GU, ZIGP_KFU_RES_GS, ZIGP_KFU_RES_SIZE, ZIGP_KFU_RES_PWS,
       ZIGP_KFU_RES_INFO, ZIGP_KFU_N_RES,
       ZIGP_KFU_GRID,                 /* workgroups of every update launch: the big ones and the hyperparameter one */
       ZIGP_KFU_BIG_OFF,              /* [9]: first element of each big block in the big workgroups' element order; [8] = their total */
       ZIGP_KFU_HYP_OFF = ZIGP_KFU_BIG_OFF + 9,    /* [10]: the same for the hyperparameter workgroup */
       ZIGP_KFU_N_IMG = ZIGP_KFU_HYP_OFF + 10,     /* doubles of the parameter image with both hyperparameter blocks */
       ZIGP_KFU_OFF_HYP, ZIGP_KFU_OFF_HYP2,        /* the block step i reads is HYP for even i, HYP2 for odd i; its update writes the other */
       ZIGP_KFU_OFF_Z,                /* [4]: image offset of Z of (latent, factor) = (0,0) (0,1) (1,0) (1,1) */
       ZIGP_KFU_OFF_U = ZIGP_KFU_OFF_Z + 4, ZIGP_KFU_OFF_S = ZIGP_KFU_OFF_U + 2,   /* [2] each */
       ZIGP_KFU_KH_SIZE = ZIGP_KFU_OFF_S + 2, ZIGP_KFU_KH_FAC, ZIGP_KFU_KH_INV, ZIGP_KFU_KH_ZC, ZIGP_KFU_KH_ELL, ZIGP_KFU_KH_VAR,
       ZIGP_KFU_KH_NOISE, ZIGP_KFU_KH_FMU,         /* layout of a hyperparameter block: record (2 h + q) * KH_FAC, slots inside it */
       ZIGP_KFU_COUNT };
typedef struct zigp_stage_kron_fit_update {
  int32_t lik;                  /* ZIGP_LIK_ONOFF, ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI */
  int32_t n_steps;
  const zigp_kron_params* shape;   /* M0f, M1f, (M0g, M1g,) D0, D1; the pointers are not read */
  const double* lr;             /* per block (17 or 10) */
  const int32_t* positive;
  const int32_t* trainable;     /* heads; NULL: every block.  Not read for ZIGP_LIK_ONOFF */
  double beta1, beta2, eps;
  int64_t t0, n_free;
  double *x, *m, *v;            /* in / out [n_free], as the fit calls */
  const double* res;            /* [n_steps][n_res] or NULL */
  int64_t n_res, n_img;         /* must equal facts' (checked when res != NULL) */
  double *snap_x, *snap_m, *snap_v;   /* out [1 + n_steps][n_free]: behind the initial image launch, then behind every update launch; any may be NULL */
  double* snap_img;             /* out [1 + n_steps][n_img], may be NULL */
  double* hist;                 /* out [n_steps][2]: the device history as downloaded (data term, KL); may be NULL */
  int32_t* fail;                /* out [4]: the device failure record {1 + step, job, pivot, -}; may be NULL */
  double *elbo_data, *kl;       /* out [n_steps]: the history as the entry points return it (NaN from a failing step on); may be NULL */
  int64_t* steps_applied;       /* out, may be NULL */
  int64_t* facts;               /* out [ZIGP_KFU_COUNT], may be NULL */
} zigp_stage_kron_fit_update;
int zigp_test_kron_fit_update(zigp_ctx* ctx, const zigp_stage_kron_fit_update* a);

/* k_dense_fit_image, k_dense_fit_image_tri and k_dense_fit_update through dense_fit_steps (mode = ZIGP_FIT_*): its descriptor, grids, launches
 * and download.  Step i takes packed + i * n_packed and info + 2 i in place of k_gather_rows + the step + k_dense_pack.  The packed vector has
 * the layout of zigp_stage_pack::out: 16 header doubles (data term, KL, d var_f, d var_g, d noise, ...), then per latent dZ (M, D), du (M),
 * ds (M; ZIGP_FIT_WHITE_FULL: the lower triangle of dLq in row-major order, M (M + 1) / 2), dell (D).  A data set must be resident
 * (zigp_set_data; any rows of the shape's D): the loop plans its step although the hook does not run it.
 * Snapshots behind every image launch (slot 0: the initial one, slot 1 + i: the one behind update i) and, for x / m / v, the same slots. */
enum { ZIGP_DFU_IMG_Z = 0,            /* [2] each: f, g */
       ZIGP_DFU_IMG_ELL = 2, ZIGP_DFU_IMG_U = 4, ZIGP_DFU_IMG_S = 6, ZIGP_DFU_IMG_ZS = 8, ZIGP_DFU_MP = 10,
       ZIGP_DFU_N_IMG = 12, ZIGP_DFU_N_PACKED, ZIGP_DFU_GRID, ZIGP_DFU_TGRID,
       ZIGP_DFU_DH_SIZE, ZIGP_DFU_DH_LAT, ZIGP_DFU_DH_INV, ZIGP_DFU_DH_ELL, ZIGP_DFU_DH_SCALE, ZIGP_DFU_DH_VAR, ZIGP_DFU_DH_PIVTOL, ZIGP_DFU_DH_NOISE,
       ZIGP_DFU_COUNT };
typedef struct zigp_stage_dense_fit_update {
  int32_t mode, n_steps;
  const zigp_params* shape;     /* Mf, Mg, D */
  const zigp_fit_opts* opts;
  int64_t t0, n_free;
  double jitter;
  double *x, *m, *v;            /* in / out [n_free] */
  const double* packed;         /* [n_steps][n_packed] or NULL: only facts is filled */
  const int32_t* info;          /* [n_steps][2] */
  int64_t n_packed, n_img;      /* must equal facts' (checked when packed != NULL) */
  double *snap_x, *snap_m, *snap_v;   /* out [1 + n_steps][n_free], any may be NULL */
  double* snap_img;             /* out [1 + n_steps][n_img]: the parameter image at its padded size */
  double* snap_H;               /* out [1 + n_steps][DH_SIZE] */
  double* snap_Lraw[2];         /* out [1 + n_steps][M_h * M_h], ZIGP_FIT_WHITE_FULL only */
  double* hist;                 /* out [n_steps][2] as downloaded */
  int32_t* fail;                /* out [4] */
  double *elbo_data, *kl;       /* out [n_steps] as the entry points return them */
  int64_t* steps_applied;
  int64_t* facts;               /* out [ZIGP_DFU_COUNT] */
} zigp_stage_dense_fit_update;
int zigp_test_dense_fit_update(zigp_ctx* ctx, const zigp_stage_dense_fit_update* a);

/* ---- The weight stage of the sample paths: what turns a draw of q(u) into the weight table the path kernels read, through the function the
 * product entry points themselves call (path_weight_stage of csrc/zigp_paths.hip, kron_path_weight_stage of csrc/zigp_kronpaths.hip) behind the
 * call's own M x M forward stage -- the same launches, grids and device buffers; the paths at Xnew are not run.  A tap is a stream-ordered
 * device-to-device copy enqueued right behind the launch that produces the value, downloaded after the stage's synchronisation, so a later
 * launch that reuses the buffer cannot matter; a NULL tap is not taken.  The work matrices a launch must write completely hold
 * ZIGP_STAGE_SENTINEL_BYTE before the stage (an ordinary call clears them to 0): an element that still holds it was not written.  Both hooks
 * synchronise, return what the entry point's factorisation check returns and leave the context usable. ---- */
/* Dense model.  Mp = M rounded up to 128, Sp = S rounded up to 128, nst = sample tiles per pass (1, 2 or 4), ntile = ceil(S / 16) rounded up
 * to nst, M4 / R4 = M / R rounded up to 4, F = M4 + R4.  "Diag" is the unwhitened parametrisation, "White" / "WhiteFull" the whitened ones. */
typedef struct zigp_pathw_tap_latent {
  double *Kuu, *W;      /* [Mp][Mp] as the call's latents_forward left them: Kuu + jitter I and W = L^-1, identity in the padding */
  double *Lq;           /* WhiteFull: [Mp][Mp] the masked lower-triangular image of L_q, zero padding */
  double *u, *s;        /* [Mp] as the device holds them, zero padding */
  double *E;            /* [Mp][Sp] the staged eps, zero outside (M, S) */
  double *FT;           /* [Sp][Mp] f_Z as the path kernel wrote it: FT[s][m], s < S, m < M; zero elsewhere */
  double *rhs;          /* [Mp][Sp] after k_path_rhs (Diag: u + s o eps - f_Z; White / WhiteFull: t); exact zero outside (M, S) */
  double *t;            /* Diag: [Mp][Sp] W rhs */
  double *V0;           /* Diag: [Mp][Sp] W^T t, the weights BEFORE the refinement step */
  double *KV;           /* Diag: Kuu V0 */
  double *res;          /* Diag: rhs - Kuu V0 (k_path_axpy) */
  double *t2, *cor;     /* Diag: W res and the correction W^T (W res) */
  double *G, *H;        /* White / WhiteFull: G = W f_Z; WhiteFull: H = tril(L_q) E */
  double *V;            /* [Mp][Sp] the final weights (Diag: V0 + cor by k_path_axpy) */
  double *tab;          /* [ntile][F][16] the weight table after k_path_fill_v: rows < M4 from V, rows M4 .. F - 1 the cosine amplitudes as the host
                           staged them.  The hook fills rows < M4 with the sentinel before k_path_fill_v */
} zigp_pathw_tap_latent;
enum { ZIGP_PWF_MODE = 0,      /* 0 Diag, 1 White, 2 WhiteFull */
       ZIGP_PWF_SP, ZIGP_PWF_NST, ZIGP_PWF_NTILE,
       ZIGP_PWF_MP,            /* [2] f, g; then M4 [2], R4 [2], F [2] */
       ZIGP_PWF_M4 = ZIGP_PWF_MP + 2, ZIGP_PWF_R4 = ZIGP_PWF_M4 + 2, ZIGP_PWF_F = ZIGP_PWF_R4 + 2,
       ZIGP_PWF_COUNT = ZIGP_PWF_F + 2 };
typedef struct zigp_stage_path_weights {
  const zigp_params* p;         /* read as zigp_sample_paths reads it (the context's parametrisation and kernels apply) */
  double jitter;
  const zigp_path_draw *draw_f, *draw_g;
  int32_t S, reserved;
  zigp_pathw_tap_latent lat[2];
  int64_t* facts;               /* out [ZIGP_PWF_COUNT], may be NULL */
} zigp_stage_path_weights;
int zigp_test_path_weights(zigp_ctx* ctx, const zigp_stage_path_weights* a);

/* Kronecker model and heads.  M = M0 M1, Mq_p = M_p rounded up to 128 (the row stride of K_p and W_p), M1p = M1 rounded up to 4,
 * F = M0 M1p + R4.  The grid matrices are [S][M0][M1] (sample-major, factor-0-major inside a sample). */
typedef struct zigp_kpathw_tap_latent {
  double *K[2], *W[2];  /* [Mq_p][Mq_p] as factor_forward left them: K_p + jitter I, W_p = L_p^-1 */
  double *E;            /* [M][S] eps as the draw holds it */
  double *U, *Sq;       /* [M] */
  double *FZ;           /* [S][M] f_Z as the path kernel wrote it */
  double *rhs;          /* [S][M] after k_kp_rhs */
  double *A1;           /* after k_kp_left:  W0 rhs_s */
  double *B1;           /* after k_kp_right: (W0 rhs_s) W1^T */
  double *A2;           /* after k_kp_left:  W0^T (..) */
  double *V;            /* after k_kp_right: (..) W1, the weights */
  double *tab;          /* [ntile][F][16] after k_kp_fill_v; the hook fills rows < M0 M1p with the sentinel before that launch */
} zigp_kpathw_tap_latent;
enum { ZIGP_KWF_NST = 0, ZIGP_KWF_NTILE,
       ZIGP_KWF_MQ0,           /* [2] f, g; then Mq1 [2], M1p [2], R4 [2], F [2] */
       ZIGP_KWF_MQ1 = ZIGP_KWF_MQ0 + 2, ZIGP_KWF_M1P = ZIGP_KWF_MQ1 + 2, ZIGP_KWF_R4 = ZIGP_KWF_M1P + 2, ZIGP_KWF_F = ZIGP_KWF_R4 + 2,
       ZIGP_KWF_COUNT = ZIGP_KWF_F + 2 };
typedef struct zigp_stage_kron_path_weights {
  const zigp_kron_params* p;
  int32_t lik;                  /* ZIGP_LIK_ONOFF (two latents) or a head (the f fields of everything) */
  int32_t S;
  double jitter;
  const zigp_path_draw *draw_f, *draw_g;      /* draw_g: ZIGP_LIK_ONOFF only */
  zigp_kpathw_tap_latent lat[2];
  int64_t* facts;               /* out [ZIGP_KWF_COUNT], may be NULL */
} zigp_stage_kron_path_weights;
int zigp_test_kron_path_weights(zigp_ctx* ctx, const zigp_stage_kron_path_weights* a);

#ifdef __cplusplus
}
#endif
#endif
