// Dense zero-inflated-GP ELBO path: host orchestration + C-ABI (include/zigp.h).
//
// Per ELBO step (value + gradient), for each latent h in {f, g}:
//   MxM stage   Kuu = k(Z,Z)+jitter I ; L = chol(Kuu) ; W = L^-1                    (OnOffSVGP.py:96-97, main.py:267-268)
//   per chunk   K = k(Z, Xc) ; A1 = W K ; column sums -> mean                          (main.py:266-303)
//               value-only / predict: A2 = W^T A1 (accumulators only) ; var = var0 - sum A1^2 + sum s^2 A2^2
//               gradient step:  H = (W diag(s^2)) A2 ; J' = W^T H - A2 = Q A2 = (Q W^T) A1   (gradient panel, independent of the cotangents)
//                               var = var0 + sum_m K J'  (k^T J' = k^T P S P k - k^T P k, P = Kuu^-1, S = diag(s^2)): no A2 product,
//                               8 M^2 N flops per step (A1, J', rank-N update) instead of 10
//               point-wise probit / likelihood / reverse pass -> gm, gv               (OnOffSVGP.py:168-204, OnOffLikelihood.py:30-32)
//               reverse of the two triangular solves, with G = diag(gv), v = W u, alpha = W^T v:
//                 E = W dA2 = v gm^T + 2 H G ;  F = dK = W^T(E - 2 A1 G) = alpha gm^T + 2 J' G
//                 dL = -tril(F A1^T + A2 E^T) = -tril(alpha (A1 gm)^T + (A2 gm) v^T + 2 [J' G A1^T + A2 G H^T])
//               and, with T = W diag(s^2) W^T (so H = T A1, J' = W^T (T - I) A1) and C1 = A1 G A1^T:
//                 J' G A1^T + A2 G H^T = W^T (T C1 + C1 T - C1)
//               so all four O(M^2 N) triangular products run back to back before the point-wise stage, and ONE
//               gv-weighted symmetric rank-N update C1 (gv applied as a k-scale inside the GEMM core, split-K,
//               fixed order) replaces the two rank-N updates of the literal reverse pass; the rest is O(M^3).
//   MxM stage   Kuu-bar = sym(W^T Phi(L^T dL) W) - dKL/dKuu ; -> dZ, dell, dvar        (Cholesky reverse, Murray 2016 / TF CholeskyGrad)
//
// Whitened parametrisation (zigp_set_whiten; GPConditional(whiten=True) skips the second back-substitution, main.py:282-284, and the white
// GaussKL has no Kuu, :193-195,227-228,246; OnOffSVGP.py:88-91,133,137).  q(u) = N(L u, L diag(s^2) L^T), D = diag(s^2 - 1), A = W K:
//   per chunk   A = W K with column sums  mean = sum_m u A ,  var = var0 + sum_m (s^2 - 1) A^2 : ONE triangular product (2 M^2 N), whose
//               panel has no reader in a value-only / predict pass (EpiColsum: never stored)
//               point-wise stage (needs the A launch only)
//               gradient step:  J' = (W^T D) A  (upper-triangular product, M^2 N) ;  F = dK = alpha gm^T + 2 J' G , alpha = W^T u  (k_kgrad
//               as it is) ;  C1 = A G A^T (the rank-N update as it is): 6 M^2 N flops per step instead of 8
//   MxM stage   du = W (K gm) - u ;  ds = 2 s diag(C1) - s + 1/s ;  dL = -tril(alpha (A gm)^T + 2 (W^T D) C1) ;  Kuu-bar = sym(W^T Phi(L^T dL) W)
//               (no P, Q, R, T, U, V; the KL adds nothing to Kuu-bar)
// The branch is taken on the host alone: an unwhitened call launches exactly what it launched before the mode existed.
//
// Full-covariance q(u) on the whitened model (zigp_set_q_full; the 3-d q_sqrt branches, OnOffSVGP.py:59-71, main.py:208-213,292-296).
// q(u) = N(L u, L Lq Lq^T L^T), Lq lower triangular (M x M), T = Lq Lq^T, R = W^T (T - I), A = W K:
//   per chunk   A = W K with column sums  mean = sum_m u A  and  sum_m A^2  (the lower-triangular launch, panel stored)
//               value-only / predict:  B = Lq^T A (upper-triangular product, accumulators only: the A2 launch with Lq where W sits and
//               weights 1) ;  var = var0 - sum A^2 + sum B^2                                           4 M^2 N flops
//               gradient step:  J' = R A (the full product of the unwhitened step, epilogue sum_m K J' = A^T (T - I) A) ;
//               var = var0 + sum_m K J' ;  F = alpha gm^T + 2 J' G, alpha = W^T u ;  C1 = A G A^T          8 M^2 N flops
//   MxM stage   forward: Lq masked and padded (k_lq_stage), KL (k_kl_white_full), T - I and R^T = (T - I) W (split-K, gradient steps)
//               backward: du = W (K gm) - u ;  dLq = tril(2 C1 Lq) - (tril(Lq) - diag(1 / Lq_ii)) ;  dL = -tril(alpha (A gm)^T + 2 R C1),
//               then the whitened chain.
// Every chunk-loop launch is an instantiation the unwhitened path already runs; only operands differ.
#include "zigp_ctx.h"
#include "zigp_kernels.h"
#include "zigp_host.h"
#include "zigp_rows.h"
#include "zigp_comm.h"
#include <algorithm>
#include <cmath>
#include <functional>

using namespace zigp;

static_assert(WIDE_MAXD == ZIGP_MAX_D, "the wide kernels' hyperparameter structs hold ZIGP_MAX_D entries");
#define ZIGP_STR2(x) #x
#define ZIGP_STR(x) ZIGP_STR2(x)
#define ZIGP_MAX_D_STR ZIGP_STR(ZIGP_MAX_D)

namespace {

// The variational parametrisation of a call -- the three models of the header comment.  One value travels with the call (DenseCall::par)
// and every host-side branch reads it; the pair "full covariance without whitening" does not exist (validate_params refuses it).
enum class Param : int { Diag = 0, White = 1, WhiteFull = 2 };
constexpr bool is_white(Param p) { return p != Param::Diag; }
constexpr bool is_full(Param p) { return p == Param::WhiteFull; }
// the `mode` of zigp_fit_steps_mode and of the stage diagnostics converts by cast, after its range check
static_assert((int)Param::Diag == ZIGP_FIT_DIAG && (int)Param::White == ZIGP_FIT_WHITE && (int)Param::WhiteFull == ZIGP_FIT_WHITE_FULL,
              "Param values are the ZIGP_FIT_* modes of include/zigp.h");
// the context's two settable flags as a Param; validate_params refuses q_full without whiten before any caller gets here
Param param_of(const zigp_ctx* c) { return !c->whiten ? Param::Diag : c->q_full ? Param::WhiteFull : Param::White; }

struct HostLatent {
  int M; const double *Z, *u, *s, *ell; double var;
  int kind = ZIGP_KERN_RBF;     // kernel family of the latent (zigp_set_kernel), read once per call next to param_of: run_dense, zigp_prior_kl
};
static_assert(KERN_RBF == ZIGP_KERN_RBF && KERN_M32 == ZIGP_KERN_MATERN32 && KERN_M52 == ZIGP_KERN_MATERN52,
              "the kernels' kind values are the ZIGP_KERN_* constants of include/zigp.h");
constexpr bool is_matern(int kind) { return kind != ZIGP_KERN_RBF; }
const char* kern_name(int kind) { return kind == ZIGP_KERN_MATERN32 ? "Matern32" : kind == ZIGP_KERN_MATERN52 ? "Matern52" : "RBF"; }
// "... Matern52 kernel on latent g ..." for the refusals that name the kernel (nullptr: both latents RBF)
const char* matern_latent(const zigp_ctx* c, std::string& who) {
  for (int h = 0; h < 2; ++h)
    if (is_matern(c->kern[h])) { who = std::string(kern_name(c->kern[h])) + " kernel on latent " + (h ? "g" : "f"); return who.c_str(); }
  return nullptr;
}

// Parameters of both latents to the device (zero-padded to Mp): ONE staged image [Z | ell | u | s | Zs] x 2 and one copy -- the eight
// separate copies of the first version were eight launches (~7 us apart) in front of a launch-bound M x M stage.  lt.Z / ell / u / s
// are views into the context's parameter arena.
// Centre of k_kgrad's moment sums (the mean inducing input) and the choice of its form, from the host copies of Z and ell
// (latents_upload; zigp_test_kgrad's defaults)
void kgrad_centre(Latent& lt, const double* Z, const double* ell, int M, int D) {
  double spread = 0.0;
  for (int d = 0; d < WIDE_MAXD; ++d) {
    double sum = 0.0;
    if (d < D) for (int m = 0; m < M; ++m) sum += Z[(size_t)m * D + d];
    lt.zc[d] = M > 0 ? sum / M : 0.0;
    if (d < D) for (int m = 0; m < M; ++m) spread = std::max(spread, std::fabs(Z[(size_t)m * D + d] - lt.zc[d]) / ell[d]);
  }
  // inducing inputs further than KG_EXACT_SPREAD lengthscales from their mean (or not finite): per-row differences instead of the shift
  lt.kg_exact = !(spread <= KG_EXACT_SPREAD);
}

// Layout of the parameter image for the sizes M (sets lat[h].M / Mp, sizes c->parm) and, once the image is in place or on its way, the
// views into it and the M x M buffers (latents_views).  latents_upload stages the image from host values; the fit loop
// (zigp_fit_steps) has k_dense_fit_image write it from the free state.
int latents_layout(zigp_ctx* c, const int (&M)[2], int D, size_t (&off)[2][6], size_t& total) {
  total = 0;
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    lt.M = M[h];
    lt.Mp = (int)round_up(M[h], BM);
    const size_t Mp = lt.Mp;
    off[h][0] = total; total += Mp * D;      // Z
    off[h][1] = total; total += std::max(D, MAXD);   // ell: max(D, 8) doubles, so every offset is what it was for D <= 8
    off[h][2] = total; total += Mp;          // u
    off[h][3] = total; total += Mp;          // s
    off[h][4] = total; total += Mp * D;      // Zs = Z scaled to k_kuf_build's units (the same doubles the kernel multiplies into x)
    off[h][5] = total;
  }
  ZIGP_ENSURE(c, c->parm, total);
  return 0;
}
int latents_views(zigp_ctx* c, const size_t (&off)[2][6], int D) {
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const size_t Mp = lt.Mp;
    lt.Z.alias(c->parm.p + off[h][0], Mp * D); lt.ell.alias(c->parm.p + off[h][1], std::max(D, MAXD));
    lt.u.alias(c->parm.p + off[h][2], Mp); lt.s.alias(c->parm.p + off[h][3], Mp); lt.Zs.alias(c->parm.p + off[h][4], Mp * D);
    ZIGP_ENSURE(c, lt.s2, Mp);
    ZIGP_ENSURE(c, lt.Kuu, Mp * Mp);
    ZIGP_ENSURE(c, lt.L, Mp * Mp);
    ZIGP_ENSURE(c, lt.W, Mp * Mp);
    ZIGP_ENSURE(c, lt.T1, Mp * Mp);
    ZIGP_ENSURE(c, lt.vec, 4 * Mp + 8);
    ZIGP_ENSURE(c, lt.wh, 4 * Mp + 8);
    ZIGP_ENSURE(c, lt.Wp, Mp * Mp);
    ZIGP_ENSURE(c, lt.Wt, Mp * Mp);
    ZIGP_ENSURE(c, lt.P, Mp * Mp); ZIGP_ENSURE(c, lt.Qt, Mp * Mp); ZIGP_ENSURE(c, lt.Rt, Mp * Mp);
  }
  return 0;
}
// WhiteFull: hl[h].s is the (M, M) row-major block; the image's s slot gets its diagonal (k_kuu_setup squares it, nobody reads the result)
// and the block itself goes to Latent::Lraw, for k_lq_stage (latents_forward) to mask and pad.
int latents_upload(zigp_ctx* c, const HostLatent (&hl)[2], int D, Param par) {
  size_t off[2][6], total = 0;
  const int M[2] = {hl[0].M, hl[1].M};
  ZIGP_TRY(latents_layout(c, M, D, off, total));
  for (int h = 0; h < 2; ++h) c->lat[h].var = hl[h].var;
  ZIGP_PINNED(c, img, total);
  memset(img, 0, sizeof(double) * total);
  for (int h = 0; h < 2; ++h) {
    const HostLatent& q = hl[h];
    memcpy(img + off[h][0], q.Z, sizeof(double) * q.M * D);
    memcpy(img + off[h][1], q.ell, sizeof(double) * D);
    memcpy(img + off[h][2], q.u, sizeof(double) * q.M);
    if (is_full(par)) for (int m = 0; m < q.M; ++m) img[off[h][3] + m] = q.s[(size_t)m * q.M + m];
    else memcpy(img + off[h][3], q.s, sizeof(double) * q.M);
    const KufHypWide kh = make_kuf_hyp_wide(q.ell, q.var, D);
    kgrad_centre(c->lat[h], q.Z, q.ell, q.M, D);
    for (int m = 0; m < q.M; ++m)
      for (int d = 0; d < D; ++d) img[off[h][4] + (size_t)m * D + d] = q.Z[(size_t)m * D + d] * kh.scale[d];
  }
  ZIGP_HIP(c, hipMemcpyAsync(c->parm.p, img, sizeof(double) * total, hipMemcpyHostToDevice, c->stream));
  if (is_full(par))
    for (int h = 0; h < 2; ++h) {
      Latent& lt = c->lat[h];
      const size_t mm = (size_t)hl[h].M * hl[h].M, mmp = (size_t)lt.Mp * lt.Mp;
      ZIGP_ENSURE(c, lt.Lraw, mm); ZIGP_ENSURE(c, lt.Lq, mmp); ZIGP_ENSURE(c, lt.lqssq, mmp / 256);
      ZIGP_PINNED(c, raw, mm);
      memcpy(raw, hl[h].s, sizeof(double) * mm);
      ZIGP_HIP(c, hipMemcpyAsync(lt.Lraw.p, raw, sizeof(double) * mm, hipMemcpyHostToDevice, c->stream));
    }
  return latents_views(c, off, D);
}

// ---- M x M stage of a full-covariance call (zigp_set_q_full), per latent, on the stream the caller selected ----
// Lraw -> the masked, padded image Lq and its block sums; then the KL and the call's small vectors (Latent::wh)
int latent_qfull_stage(zigp_ctx* c, Latent& lt) {
  const int Mp = lt.Mp, nblk = (int)((size_t)Mp * Mp / 256);
  hipLaunchKernelGGL(k_lq_stage, dim3(nblk), dim3(256), 0, c->stream, lt.Lraw.p, lt.M, (int64_t)Mp, lt.Lq.p, lt.lqssq.p);
  hipLaunchKernelGGL(k_kl_white_full, dim3(1), dim3(256), 0, c->stream, lt.u.p, lt.Lq.p, lt.lqssq.p, nblk, lt.M, (int64_t)Mp, lt.wh.p);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
// T - I = Lq Lq^T - I -> P (both factors lower triangular: k <= min(i, j)), then R^T = (T - I) W -> Rt (W lower triangular: k >= j), the
// image the J' launch reads and the left factor of R C1 in the reverse stage
int latent_qfull_factors(zigp_ctx* c, Latent& lt) {
  const int Mp = lt.Mp, nb = Mp / BM;
  ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_KCONTIG>(c, lt.sk, SkRule::TT, nb, lt.Lq.p, lt.Lq.p, lt.P.p, Mp, SK_STORE, 1.0)));
  hipLaunchKernelGGL(k_sub_eye, dim3(ceil_div(Mp, 256)), dim3(256), 0, c->stream, lt.P.p, lt.M, (int64_t)Mp);
  ZIGP_HIP(c, hipGetLastError());
  return run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::Y, nb, lt.P.p, lt.W.p, lt.Rt.p, Mp, SK_STORE, 1.0);
}
// dLq = tril(2 C1 Lq) - [kl] (tril(Lq) - diag(1 / Lq_ii)) -> dLq ; C1 in T1 (with_data), Y = C1 Lq -> T3
int latent_qfull_dlq(zigp_ctx* c, Latent& lt, bool with_data, bool with_kl) {
  const int Mp = lt.Mp, nb = Mp / BM;
  const size_t mm = (size_t)Mp * Mp;
  ZIGP_ENSURE(c, lt.T3, mm); ZIGP_ENSURE(c, lt.dLq, mm);
  if (with_data)
    ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::Y, nb, lt.T1.p, lt.Lq.p, lt.T3.p, Mp, SK_STORE, 1.0)));
  hipLaunchKernelGGL(k_dlq_assemble, dim3(ceil_div((int64_t)mm, 256)), dim3(256), 0, c->stream, lt.T3.p, lt.Lq.p, with_data ? 1 : 0, with_kl ? 1 : 0,
                     lt.M, (int64_t)Mp, lt.dLq.p);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

// MxM forward of BOTH latents (kernels only): Kuu, L = chol, W = L^-1 (+ W^T), the KL pieces v = W u,
// alpha = W^T v, dkinv = diag(K^-1), kl -> vec[3*Mp], and W' = W diag(s^2) for gradient steps.  Latent f runs on the main stream and g
// on stream2 (the caller forks / joins); the launches ALTERNATE between the two chains step by step, so that both streams are fed
// from the start (see potrf_trtri_jobs).
// d_hyp (fit loop, zigp_fit_steps): the hyperparameters and the pivot tolerances come from this device block (zigp_kernels.h, DH_*), hl
// carries the sizes only, and latent h reports a failed factorisation in d_info2[h].
// White: W^T, alpha = W^T u (gradient steps), the white KL and the call's whitened vectors (k_kl_white -> Latent::wh) and, for gradient
// steps, D W = diag(s^2 - 1) W in `Wp`, the factor image of J' = (W^T D) A and of the reverse stage's (W^T D) C1; no v, P, Q or R.
// WhiteFull: the staged factor and its KL in place of k_kl_white, and T - I, R^T in place of D W (latent_qfull_*).
int latents_forward(zigp_ctx* c, const HostLatent (&hl)[2], int D, double jitter, Param par, bool with_kl, bool need_grad, const double* d_hyp,
                    int* d_info2) {
  const hipStream_t st[2] = {c->stream_main, c->stream2};
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const int Mp = lt.Mp;
    OnStream on(c, st[h]);
    const dim3 grid(ceil_div((int64_t)Mp * Mp, 256));
    if (is_matern(hl[h].kind))     // D <= MAXD and no device block: validate_params and dense_fit_steps refuse the rest
      hipLaunchKernelGGL(k_kuu_setup_matern, grid, dim3(256), 0, c->stream, lt.Z.p, (int64_t)hl[h].M, make_hyp(hl[h].ell, hl[h].var, D), hl[h].kind, jitter,
                         lt.Kuu.p, lt.L.p, lt.W.p, lt.s.p, lt.s2.p, (int64_t)Mp);
    else if (d_hyp)
      hipLaunchKernelGGL(k_kuu_setup<LatHypDev>, grid, dim3(256), 0, c->stream, lt.Z.p, (int64_t)hl[h].M, LatHypDev{d_hyp + h * DH_LAT, D}, jitter, lt.Kuu.p,
                         lt.L.p, lt.W.p, lt.s.p, lt.s2.p, (int64_t)Mp);
    else if (D > MAXD)
      hipLaunchKernelGGL(k_kuu_setup<KernHypWide>, grid, dim3(256), 0, c->stream, lt.Z.p, (int64_t)hl[h].M, make_hyp_wide(hl[h].ell, hl[h].var, D), jitter,
                         lt.Kuu.p, lt.L.p, lt.W.p, lt.s.p, lt.s2.p, (int64_t)Mp);
    else {
      KernHyp hyp = make_hyp(hl[h].ell, hl[h].var, D);
      hipLaunchKernelGGL(k_kuu_setup<KernHyp>, grid, dim3(256), 0, c->stream, lt.Z.p, (int64_t)hl[h].M, hyp, jitter, lt.Kuu.p,
                         lt.L.p, lt.W.p, lt.s.p, lt.s2.p, (int64_t)Mp);
    }
    ZIGP_HIP(c, hipGetLastError());
  }
  {
    PotrfJob jobs[2];
    for (int h = 0; h < 2; ++h) {
      Latent& lt = c->lat[h];
      jobs[h] = PotrfJob{lt.L.p, lt.W.p, lt.T1.p, lt.Mp, true, lt.M, d_hyp ? 0.0 : pivot_tol(hl[h].var, jitter, c->pivot_rtol), true, &lt.sk};
      if (d_hyp) { jobs[h].tol_dev = d_hyp + h * DH_LAT + DH_PIVTOL; jobs[h].info = d_info2 + h; }
    }
    ZIGP_TRY(potrf_trtri_jobs(c, 2, jobs, st));
  }
  for (int step = 0; step < 8; ++step)
    for (int h = 0; h < 2; ++h) {
      Latent& lt = c->lat[h];
      const int Mp = lt.Mp;
      OnStream on(c, st[h]);
      if (step == 0) lt.P_ready = false;
      double* v = lt.vec.p; double* alpha = v + Mp; double* dkinv = v + 2 * Mp; double* klv = v + 3 * Mp;
      if (is_white(par)) {
        switch (step) {
          case 0: hipLaunchKernelGGL(k_transpose, dim3(Mp / 32, Mp / 32), dim3(32, 8), 0, c->stream, lt.W.p, (int64_t)Mp, lt.Wt.p); break;
          case 1:
            if (is_full(par)) ZIGP_TRY(latent_qfull_stage(c, lt));
            else hipLaunchKernelGGL(k_kl_white, dim3(1), dim3(256), 0, c->stream, lt.u.p, lt.s.p, lt.M, (int64_t)Mp, lt.wh.p);
            break;
          case 2: if (need_grad) hipLaunchKernelGGL(k_gemv_cols, dim3(Mp / 64), dim3(64, COL_LANES), 0, c->stream, lt.W.p, lt.u.p, (int64_t)Mp, alpha); break;
          case 3:
            if (need_grad && is_full(par)) ZIGP_TRY(latent_qfull_factors(c, lt));
            else if (need_grad) hipLaunchKernelGGL(k_rowscale, dim3(ceil_div((int64_t)Mp * Mp, 256)), dim3(256), 0, c->stream, lt.W.p, lt.wh.p, (int64_t)Mp, lt.Wp.p);
            break;
          default: break;
        }
        ZIGP_HIP(c, hipGetLastError());
        continue;
      }
      switch (step) {
        case 0:   // W^T: the m-contiguous image of the factor that the lower-triangular product A1 = W K reads
          hipLaunchKernelGGL(k_transpose, dim3(Mp / 32, Mp / 32), dim3(32, 8), 0, c->stream, lt.W.p, (int64_t)Mp, lt.Wt.p);
          break;
        // v = W u and alpha = W^T v are needed by the KL value, by the fused mean (v^T A1) and by the rank-1 parts of the data-term gradient
        case 1: if (with_kl) hipLaunchKernelGGL(k_gemv_rows, dim3(Mp), dim3(256), 0, c->stream, lt.W.p, lt.u.p, (int64_t)Mp, v); break;
        case 2: if (with_kl) hipLaunchKernelGGL(k_kl_cols, dim3(Mp / 64), dim3(64, COL_LANES), 0, c->stream, lt.W.p, v, (int64_t)Mp, alpha, dkinv); break;
        case 3: if (with_kl) hipLaunchKernelGGL(k_kl_value, dim3(1), dim3(256), 0, c->stream, v, lt.L.p, lt.s.p, dkinv, lt.M, (int64_t)Mp, klv); break;
        case 4:   // W' = W diag(s^2) (operand of the reverse M x M stage)
          if (need_grad) hipLaunchKernelGGL(k_colscale, dim3(ceil_div((int64_t)Mp * Mp, 256)), dim3(256), 0, c->stream, lt.W.p, lt.s2.p, (int64_t)Mp, lt.Wp.p);
          break;
        case 5:   // P = W^T W = Kuu^-1 (the reverse M x M stage needs it anyway and takes it from here)
          if (need_grad) {
            ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::S, Mp / BM, lt.W.p, lt.W.p, lt.P.p, Mp, SK_STORE, 1.0)));
            lt.P_ready = true;
          }
          break;
        case 6:   // Q^T = diag(s^2) P - I: J' = W^T (W diag(s^2) A2) - A2 = (P diag(s^2) - I) A2 = Q A2 is ONE full product per chunk
          if (need_grad) hipLaunchKernelGGL(k_rowscale_minus_eye, dim3(ceil_div((int64_t)Mp * Mp, 256)), dim3(256), 0, c->stream, lt.P.p, lt.s2.p, (int64_t)Mp, lt.Qt.p);
          break;
        case 7:   // R^T = W Q^T (W lower triangular: k blocks 0 .. bi): J' = Q (W^T A1) = (Q W^T) A1 reads the A1 panel, so that the A2 panel
                  // has no reader left and is never written (r6; 8 Mp Nc bytes per latent and chunk, the A2 product 66 -> 69 TFLOP/s)
          if (need_grad) ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::RT, Mp / BM, lt.W.p, lt.Qt.p, lt.Rt.p, Mp, SK_STORE, 1.0)));
          break;
        default: break;
      }
      ZIGP_HIP(c, hipGetLastError());
    }
  return 0;
}

// Kuf panel of one latent for the chunk starting at row n0 (HBM-write bound; runs on the side stream under the previous chunk's SYRKs)
// R (fit loop): the latent's record of the device hyperparameter block; ell_host is then not read
// kind (a Matern latent; D <= MAXD, no device block): k_kuf_build_matern on the same grid; with_kd (its gradient steps): the launch also
// writes the derivative panel K' into lt.Kd (sized by dense_prepare_buffers)
int latent_chunk_kuf_matern(zigp_ctx* c, Latent& lt, const double* dX, int64_t Nrows, int64_t n0, int64_t Nc, int D, const double* ell_host, int kind,
                            bool with_kd) {
  if (D < 1 || D > MAXD || !ell_host) return fail_arg(c, "a Matern Kuf panel needs 1 <= D <= 8 and host lengthscales");
  if (with_kd && lt.Kd.cap < (size_t)lt.Mp * Nc) return fail_arg(c, "a Matern gradient step's K' panel was not sized for this chunk");
  const KufHyp kh = make_kuf_hyp(ell_host, lt.var, D);
  ProfScope ps(c, PC_KUF);
  const dim3 grid((unsigned)(Nc / 512), lt.Mp / 16), block(256);
#define ZIGP_KUF_M(DD, KK, GG) \
  hipLaunchKernelGGL((k_kuf_build_matern<DD, KK, GG>), grid, block, 0, c->stream, dX, Nrows, n0, lt.Zs.p, lt.M, kh, lt.K.p, GG ? lt.Kd.p : nullptr, Nc)
#define ZIGP_KUF_MD(DD)                                                                    \
  case DD:                                                                                 \
    if (kind == ZIGP_KERN_MATERN32) { if (with_kd) ZIGP_KUF_M(DD, KERN_M32, true); else ZIGP_KUF_M(DD, KERN_M32, false); } \
    else { if (with_kd) ZIGP_KUF_M(DD, KERN_M52, true); else ZIGP_KUF_M(DD, KERN_M52, false); }                            \
    break;
  switch (D) { ZIGP_KUF_MD(1) ZIGP_KUF_MD(2) ZIGP_KUF_MD(3) ZIGP_KUF_MD(4) ZIGP_KUF_MD(5) ZIGP_KUF_MD(6) ZIGP_KUF_MD(7) ZIGP_KUF_MD(8) }
#undef ZIGP_KUF_MD
#undef ZIGP_KUF_M
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
int latent_chunk_kuf(zigp_ctx* c, Latent& lt, const double* dX, int64_t Nrows, int64_t n0, int64_t Nc, int D, const double* ell_host,
                     const double* R = nullptr, int kind = ZIGP_KERN_RBF, bool with_kd = false) {
  if (is_matern(kind)) return latent_chunk_kuf_matern(c, lt, dX, Nrows, n0, Nc, D, ell_host, kind, with_kd);
  const int Mp = lt.Mp;
  const KufHyp kh = (R || D > MAXD) ? KufHyp() : make_kuf_hyp(ell_host, lt.var, D);
  ProfScope ps(c, PC_KUF);
  const dim3 grid((unsigned)(Nc / 512), Mp / 16), block(256);
#define ZIGP_KUF(DD)                                                                                                                   \
  case DD:                                                                                                                             \
    if (R) hipLaunchKernelGGL((k_kuf_build<DD, LatHypDev>), grid, block, 0, c->stream, dX, Nrows, n0, lt.Zs.p, lt.M, LatHypDev{R, DD}, lt.K.p, Nc); \
    else hipLaunchKernelGGL((k_kuf_build<DD, KufHyp>), grid, block, 0, c->stream, dX, Nrows, n0, lt.Zs.p, lt.M, kh, lt.K.p, Nc);               \
    break;
  switch (D) {
    ZIGP_KUF(1) ZIGP_KUF(2) ZIGP_KUF(3) ZIGP_KUF(4) ZIGP_KUF(5) ZIGP_KUF(6) ZIGP_KUF(7) ZIGP_KUF(8)
    default:      // 9 .. ZIGP_MAX_D: the run-time-D kernel, hyperparameters by value (the fit loop's device block stops at MAXD)
      if (D < 1 || D > WIDE_MAXD || R) return fail_arg(c, "D out of range");
      hipLaunchKernelGGL(k_kuf_build_wide, grid, block, 0, c->stream, dX, Nrows, n0, lt.Zs.p, lt.M, D, make_kuf_hyp_wide(ell_host, lt.var, D), lt.K.p, Nc);
      break;
  }
#undef ZIGP_KUF
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

// The launches of one chunk shape, decided on the host alone by chunk_plan (zigp_test_trmm_list checks these very lists): paired units +
// merged launches where both latents' units fill waves of the 512 slots (trmm_paired_pays), then the plan for a last wave that is not full
// (trmm_tail_plan; merged launch = [f's units | g's units], unit counts multiples of 8); per latent the lists of A1, of A2 (value-only ELBO,
// predict) or J' (gradient step) and of the rank-N update, and the flop counts the ProfScopes report.  run_dense plans and uploads
// (upload_plan) every chunk shape of a call before it enqueues anything: no hipMalloc or synchronous copy falls inside the chunk loop.  The
// tile cache keeps its lists until zigp_destroy; they follow from (Mp_f, Mp_g, Nc): at most 128 chunk sizes per M pair under the automatic
// rule, 1024 with zigp_set_chunk (multiples of 1024 rows up to 131072 / 2^20).
struct ChunkPlan {
  int64_t Nc = 0;
  bool paired = false;   // and merged: each forward product is ONE launch for both latents
  TrmmTail tail = {{0, 0}, {64, 64}};
  struct Lat { TileSpec a1_spec, a2j_spec, syr_spec, mom_spec; TileList a1, a2j, syr, mom; double fl = 0.0; } lat[2];   // a2j: A2 or J'; fl = M^2 Nc;
                                                                                             // mom: moments product of the wide Kuf gradient (D > MAXD)
};
// Every parametrisation runs A1 = W K on the same lower-triangular list; what follows it is written out per case:
//   Diag       value-only / predict: A2 = W^T A1, upper-triangular (sums only);  gradient step: J' = (Q W^T) A1 as ONE full product + the rank-N update
//   White      value-only / predict: no second product at all (a2j stays empty);  gradient step: J' = (W^T D) A, UPPER-triangular (the paired /
//              tail lists of A2) + the rank-N update
//   WhiteFull  the lists of Diag in both modes -- A and B = Lq^T A are the A1 / A2 pair, J' = R A is the full product
ChunkPlan chunk_plan(const int (&M)[2], int64_t Nc, Param par, bool need_grad, bool tail_on, bool wide) {
  ChunkPlan pl;
  const int nbm[2] = {ceil_div(M[0], BM), ceil_div(M[1], BM)}, nbn = (int)(Nc / BN);
  pl.Nc = Nc;
  pl.paired = trmm_paired_pays(nbn * ((nbm[0] + 1) / 2 + (nbm[1] + 1) / 2));
  if (pl.paired && tail_on)
    pl.tail = trmm_tail_plan((nbn + 7) / 8 * 8 * ((nbm[0] + 1) / 2), nbm[0], (nbn + 7) / 8 * 8 * ((nbm[1] + 1) / 2), nbm[1]);
  for (int h = 0; h < 2; ++h) {
    ChunkPlan::Lat& L = pl.lat[h];
    auto tri = [&](bool lower) { return trmm_tiles(lower, nbm[h], nbn, pl.paired, pl.tail.units[h], pl.tail.bins[h]); };
    auto full_product = [&] { return full_xcd_tiles(nbm[h], nbn, nbm[h] * (BM / BK)); };
    L.a1_spec = tri(true);
    switch (par) {
      case Param::Diag: L.a2j_spec = need_grad ? full_product() : tri(false); break;
      case Param::White: if (need_grad) L.a2j_spec = tri(false); break;
      case Param::WhiteFull: L.a2j_spec = need_grad ? full_product() : tri(false); break;
    }
    if (need_grad) L.syr_spec = syr2k_tiles(nbm[h], (int)(Nc / BK), syr_plan(nbm[h]));
    if (need_grad && wide) L.mom_spec = kgmom_tiles(nbm[h], Nc);
    L.fl = (double)M[h] * M[h] * (double)Nc;
  }
  return pl;
}
int upload_plan(zigp_ctx* c, ChunkPlan& pl) {
  for (ChunkPlan::Lat& L : pl.lat) {
    ZIGP_TRY(get_tiles(c, L.a1_spec, L.a1));
    if (L.a2j_spec.build) ZIGP_TRY(get_tiles(c, L.a2j_spec, L.a2j));
    if (L.syr_spec.build) ZIGP_TRY(get_tiles(c, L.syr_spec, L.syr));
    if (L.mom_spec.build) ZIGP_TRY(get_tiles(c, L.mom_spec, L.mom));
  }
  return 0;
}

// Forward panels of both latents for one chunk and their column partials: A1 and A2 (value-only ELBO, predict) or A1 and J' (gradient step).
// A gradient step launches no A2 product: the variance's  sum s^2 A2^2 - sum A1^2  is  sum_m K J'  (EpiStorePanelKColsum), reduced in the
// epilogue of the J' product the reverse pass needs anyway -- 8 M^2 N flops per step instead of 10.
// Where the triangular products run the paired order (trmm_paired_pays: cfg3, cfg2), each product class is ONE launch for both latents (run_gemm
// with two sets: g's workgroups fill the tail of f's, three launch boundaries fewer per chunk; cfg3 -0.4 ... -0.8 % same-box, profiles/r05l_ab_merge_fg.log,
// r05s_ab_milestones.log).  In the LPT regime the products stay per latent, in the order A1 A2 / A1 J' (f), then (g) (merged there: cfg2 +1.2 %), and
// so does the rank-N update everywhere (its 512-workgroup split-K plan fills the chip exactly; merged +0.2 %).
// WhiteFull (zigp_set_q_full): the same launches on the full-covariance operands -- the mean weights are u (Latent::wh), the second product's
// factor is Lq (B = Lq^T A, weights 1) or R^T = (T - I) W (J' = R A, latent_qfull_factors wrote it where Q W^T's image lies).
int chunk_forward(zigp_ctx* c, const ChunkPlan& pl, Param par, bool need_grad, const std::function<int()>& after_a1 = nullptr) {
  const int64_t Nc = pl.Nc;
  struct Set { TileList t1, t2; double fl; GemmArgs a1, a2j; EpiStoreColsum e1; EpiColsum e2; EpiStorePanelKColsum ej; } q[3] = {};   // q[2]: none
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const int Mp = lt.Mp, np = Mp / 32;   // np: allocated partial rows per fused column sum (a kernel writes one per wave tile: 64 or 32 rows)
    q[h].t1 = pl.lat[h].a1; q[h].t2 = pl.lat[h].a2j; q[h].fl = pl.lat[h].fl;
    // A1 = W K ; partial column sums  v^T A1 (= mean, since A2^T u = A1^T W u)  and  sum A1^2
    q[h].a1 = mk_args(lt.Wt.p, Mp, lt.K.p, Nc, lt.A1.p, Nc);
    q[h].e1 = EpiStoreColsum{is_full(par) ? lt.wh.p + Mp : lt.vec.p, nullptr, lt.part.p, lt.part.p + (size_t)np * Nc};
    if (need_grad) {
      // J' = Q A2 = (Q W^T) A1, Q = Kuu^-1 diag(s^2) - I (M x M, dense): the two triangular products H = W diag(s^2) A2, J' = W^T H - A2 of the
      // reverse pass as ONE full product of the same flop count -- every tile the full k range (no triangular padding, half as many prologues and
      // epilogues per flop), no H panel written and read back (r4: J' 61.9 -> 70.2 TFLOP/s, step -3.8 %, profiles/r04ak_ab_qform.log; the
      // two-product form is in tools/r4_experiment_arms.patch).  r6: with R = Q W^T formed once per step in the M x M stage (latents_forward)
      // the product reads the A1 panel, not A2.  Its epilogue also reduces sum_m K J' into plane 2 (in place of the A2 product's sums).
      q[h].a2j = mk_args(lt.Rt.p, Mp, lt.A1.p, Nc, lt.Jp.p, Nc);
      q[h].ej = EpiStorePanelKColsum{lt.K.p, lt.part.p + (size_t)2 * np * Nc};
    } else {
      // A2 = W^T A1 ; partial column sums  sum s^2 A2^2 -- the sums only: the panel has no reader (no C; ldc = stride of the partial rows)
      q[h].a2j = mk_args(is_full(par) ? lt.Lq.p : lt.W.p, Mp, lt.A1.p, Nc, nullptr, Nc);
      q[h].e2 = EpiColsum{nullptr, is_full(par) ? nullptr : lt.s2.p, nullptr, lt.part.p + (size_t)2 * np * Nc};
    }
  }
  const int groups = pl.paired ? 1 : 2;      // launch groups: merged {f, g}; LPT {f} then {g}
  for (int gi = 0; gi < groups; ++gi) {
    const Set& x = q[gi];
    const Set& y = q[pl.paired ? 1 : 2];
    {
      ProfScope ps(c, PC_GEMM_A1, x.fl + y.fl);
      ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false, TRI_A_LOWER>(c, x.t1, x.a1, x.e1, y.t1, y.a1, y.e1)));
    }
    if (gi == groups - 1 && after_a1) ZIGP_TRY(after_a1());     // the Kuf panels have had their only reader of a value-only / predict pass
    if (need_grad) {
      ProfScope ps(c, PC_GEMM_J, 2.0 * (x.fl + y.fl));
      ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false>(c, x.t2, x.a2j, x.ej, y.t2, y.a2j, y.ej)));
    } else {
      ProfScope ps(c, PC_GEMM_A2, x.fl + y.fl);
      ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false, TRI_A_UPPER>(c, x.t2, x.a2j, x.e2, y.t2, y.a2j, y.e2)));
    }
  }
  return 0;
}

// Whitened forward products of one chunk, in two parts around the point-wise stage (which needs part A alone).
// Part A: A = W K, the lower-triangular merged launch of the unwhitened path with the epilogue weights w1 = u, w2 = s^2 - 1 (Latent::wh; 0 for
// rows m >= M): plane 0 = sum_m u A (the mean, A^T u: main.py:287 without the back-substitution of :284), plane 2 = sum_m (s^2 - 1) A^2 (the
// variance's data-dependent part, :278 + :302) -- plane 2, not 1, so that the point-wise stage is k_pointwise's var = var0 + (plane 2) form.
// A gradient step stores the panel (J', the rank-N update read it); a value-only or predict pass has no reader for it and instantiates the
// same kernel with the non-storing EpiColsum: no A panel is written or even allocated there.
// Part J (gradient steps): J' = (W^T D) A -- run_gemm<TRI_A_UPPER> on the paired / tail lists of A2, the factor image D W from the M x M
// forward, a plain panel-storing epilogue (the variance needs nothing from it): M^2 Nc flops per latent, half of the unwhitened J'.
int chunk_forward_white(zigp_ctx* c, const ChunkPlan& pl, bool need_grad, bool part_j, const std::function<int()>& after_a = nullptr) {
  const int64_t Nc = pl.Nc;
  struct Set { TileList t; double fl; GemmArgs g; EpiStoreColsum es; EpiColsum ec; } q[3] = {};   // q[2]: none
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const int Mp = lt.Mp, np = Mp / 32;
    double* p0 = lt.part.p; double* p2 = lt.part.p + (size_t)2 * np * Nc;
    q[h].fl = pl.lat[h].fl;
    if (part_j) { q[h].t = pl.lat[h].a2j; q[h].g = mk_args(lt.Wp.p, Mp, lt.A1.p, Nc, lt.Jp.p, Nc); continue; }
    q[h].t = pl.lat[h].a1;
    q[h].g = mk_args(lt.Wt.p, Mp, lt.K.p, Nc, need_grad ? lt.A1.p : nullptr, Nc);
    q[h].es = EpiStoreColsum{lt.wh.p + Mp, lt.wh.p, p0, p2};
    q[h].ec = EpiColsum{lt.wh.p + Mp, lt.wh.p, p0, p2};
  }
  const int groups = pl.paired ? 1 : 2;      // launch groups: merged {f, g}; LPT {f} then {g}
  for (int gi = 0; gi < groups; ++gi) {
    const Set& x = q[gi];
    const Set& y = q[pl.paired ? 1 : 2];
    if (part_j) {
      ProfScope ps(c, PC_GEMM_J, x.fl + y.fl);
      ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false, TRI_A_UPPER>(c, x.t, x.g, EpiStore(), y.t, y.g, EpiStore())));
      continue;
    }
    {
      ProfScope ps(c, PC_GEMM_A1, x.fl + y.fl);
      if (need_grad) ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false, TRI_A_LOWER>(c, x.t, x.g, x.es, y.t, y.g, y.es)));
      else ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false, TRI_A_LOWER>(c, x.t, x.g, x.ec, y.t, y.g, y.ec)));
    }
    if (gi == groups - 1 && after_a) ZIGP_TRY(after_a());     // the Kuf panels have had their only reader of a value-only / predict pass
  }
  return 0;
}

// D > MAXD, centred form: T over J' and the operand XM (k_kgrad_wide_prep), the moments product on the GEMM core, the planes into krow.
// `mom` is the chunk shape's planned list (ChunkPlan::Lat::mom); the buffers were sized before the loop (dense_prepare_buffers).
int latent_chunk_kgrad_wide(zigp_ctx* c, Latent& lt, const double* dX, int64_t Nrows, int64_t n0, int64_t Nc, int D, const TileList& mom) {
  const int Mp = lt.Mp, S = kgmom_slices(Mp / BM, Nc);
  if (mom.n != S * (Mp / BM)) return fail_arg(c, "wide Kuf gradient: the moments product's tile list was not planned for this chunk shape");
  KgCentreWide ctr;
  for (int d = 0; d < WIDE_MAXD; ++d) ctr.c[d] = lt.zc[d];
  hipLaunchKernelGGL(k_kgrad_wide_prep, dim3(Mp / KG_ROWS, KG_SPLIT), dim3(256), 0, c->stream, lt.Jp.p, lt.K.p, lt.vec.p + Mp, lt.gm.p, lt.gv.p, dX, Nrows,
                     n0, lt.M, Mp, D, Nc, (int64_t)Mp * (2 + 2 * D), ctr, lt.krow.p, lt.ks0.p, lt.xm.p);
  ZIGP_HIP(c, hipGetLastError());
  GemmArgs g = mk_args(lt.Jp.p, Nc, lt.xm.p, WIDE_MOM_COLS, lt.mom.p, WIDE_MOM_COLS);
  g.slice_stride = (int64_t)Mp * WIDE_MOM_COLS;
  ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_MNCONTIG, false>(c, mom, g, EpiStore())));
  hipLaunchKernelGGL(k_kgrad_wide_finish, dim3(Mp / 4), dim3(256), 0, c->stream, lt.mom.p, S, lt.ks0.p, lt.Z.p, lt.M, Mp, D, ctr, lt.krow.p);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
int ensure_kgrad_wide(zigp_ctx* c, Latent& lt, int64_t Nc) {
  const int Mp = lt.Mp;
  ZIGP_ENSURE(c, lt.xm, (size_t)Nc * WIDE_MOM_COLS);
  ZIGP_ENSURE(c, lt.mom, (size_t)kgmom_slices(Mp / BM, Nc) * Mp * WIDE_MOM_COLS);
  ZIGP_ENSURE(c, lt.ks0, (size_t)KG_SPLIT * Mp);
  return 0;
}

// Kuf-cotangent reductions of one latent and chunk (HBM-read bound; runs on the side stream under the chunk's SYRKs)
// A Matern latent (D <= MAXD): k_kgrad_matern, the per-row form reading K and the derivative panel lt.Kd.  The centred form is not
// needed here: it exists to save fp64 VALU instructions beside the rank-N updates, and the Matern reduction already reads a third panel.
int latent_chunk_kgrad_matern(zigp_ctx* c, Latent& lt, const double* dX, int64_t Nrows, int64_t n0, int64_t Nc, int D) {
  const int Mp = lt.Mp;
  if (D < 1 || D > MAXD) return fail_arg(c, "a Matern Kuf gradient needs 1 <= D <= 8");
  if (lt.Kd.cap < (size_t)Mp * Nc) return fail_arg(c, "a Matern gradient step's K' panel was not sized for this chunk");
  ProfScope ps(c, PC_RED);
  const dim3 gk((unsigned)ceil_div(lt.M, KG_ROWS), KG_SPLIT), bk(256);
  const int64_t slab = (int64_t)Mp * (2 + 2 * D);
#define ZIGP_KGRAD_M(DD)                                                                                                                         \
  case DD:                                                                                                                                       \
    hipLaunchKernelGGL((k_kgrad_matern<DD>), gk, bk, 0, c->stream, lt.Jp.p, lt.K.p, lt.Kd.p, lt.vec.p + Mp, lt.gm.p, lt.gv.p, dX, Nrows, n0, lt.Z.p, \
                       lt.M, Nc, slab, lt.krow.p);                                                                                               \
    break;
  switch (D) { ZIGP_KGRAD_M(1) ZIGP_KGRAD_M(2) ZIGP_KGRAD_M(3) ZIGP_KGRAD_M(4) ZIGP_KGRAD_M(5) ZIGP_KGRAD_M(6) ZIGP_KGRAD_M(7) ZIGP_KGRAD_M(8) }
#undef ZIGP_KGRAD_M
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
int latent_chunk_kgrad(zigp_ctx* c, Latent& lt, const double* dX, int64_t Nrows, int64_t n0, int64_t Nc, int D, const double* ell_host,
                       const TileList& mom = TileList(), int kind = ZIGP_KERN_RBF) {
  if (is_matern(kind)) return latent_chunk_kgrad_matern(c, lt, dX, Nrows, n0, Nc, D);
  const int Mp = lt.Mp;
  KgCentre hyp;     // (not read by the wide launches)
  for (int d = 0; d < MAXD; ++d) hyp.c[d] = lt.zc[d];
  double* alpha = lt.vec.p + Mp;
  {
    ProfScope ps(c, PC_RED);
    const dim3 gk((unsigned)ceil_div(lt.M, KG_ROWS), KG_SPLIT), bk(256);
    const int64_t slab = (int64_t)Mp * (2 + 2 * D);
#define ZIGP_KGRAD(DD)                                                                                                            \
  case DD:                                                                                                                        \
    if (lt.kg_exact)                                                                                                              \
      hipLaunchKernelGGL((k_kgrad<DD, true>), gk, bk, 0, c->stream, lt.Jp.p, lt.K.p, alpha, lt.gm.p, lt.gv.p, dX, Nrows, n0, lt.Z.p, lt.M, Nc, \
                         slab, hyp, lt.krow.p);                                                                                   \
    else                                                                                                                          \
      hipLaunchKernelGGL((k_kgrad<DD, false>), gk, bk, 0, c->stream, lt.Jp.p, lt.K.p, alpha, lt.gm.p, lt.gv.p, dX, Nrows, n0, lt.Z.p, lt.M, Nc, \
                         slab, hyp, lt.krow.p);                                                                                   \
    break;
    switch (D) {
      ZIGP_KGRAD(1) ZIGP_KGRAD(2) ZIGP_KGRAD(3) ZIGP_KGRAD(4) ZIGP_KGRAD(5) ZIGP_KGRAD(6) ZIGP_KGRAD(7) ZIGP_KGRAD(8)
      default:      // 9 .. ZIGP_MAX_D: the centred moments on the GEMM core, or (lt.kg_exact) the per-row form over windows of WIDE_SLICE
                    // dimensions, one launch each
        if (D < 1 || D > WIDE_MAXD) return fail_arg(c, "D out of range");
        if (!lt.kg_exact) { ZIGP_TRY(latent_chunk_kgrad_wide(c, lt, dX, Nrows, n0, Nc, D, mom)); break; }
        for (int d0 = 0; d0 < D; d0 += WIDE_SLICE)
          hipLaunchKernelGGL(k_kgrad_slice, gk, bk, 0, c->stream, lt.Jp.p, lt.K.p, alpha, lt.gm.p, lt.gv.p, dX, Nrows, n0, lt.Z.p, lt.M, D, d0, Nc,
                             slab, lt.krow.p);
        break;
    }
#undef ZIGP_KGRAD
    ZIGP_HIP(c, hipGetLastError());
  }
  return 0;
}

// Rank-N update of the lower-triangular cotangent of one latent and chunk
int latent_chunk_syrk(zigp_ctx* c, const ChunkPlan& pl, int h) {
  Latent& lt = c->lat[h];
  const int Mp = lt.Mp;
  const int64_t Nc = pl.Nc;
  ProfScope ps(c, PC_SYR2K, pl.lat[h].fl);   // planes += tril(A1 G A1^T)   (G = diag(gv) applied as k-scale on the B operand)
  GemmArgs g = mk_args(lt.A1.p, Nc, lt.A1.p, Nc, lt.dLpart.p, Mp);
  g.slice_stride = (int64_t)Mp * Mp; g.kscale = lt.gv.p;
  return run_gemm<LAY_KCONTIG, LAY_KCONTIG, true, TRI_C_LOWER>(c, pl.lat[h].syr, g, EpiAccum());
}

// C1 = sym(sum_s planes) -> T1: the split-K planes of the chunks' rank-N updates, added in slice order
void latent_sym_from_planes(zigp_ctx* c, Latent& lt) {
  const int Mp = lt.Mp;
  const SyrPlan sp = syr_plan(Mp / BM);
  const int nt = Mp / 32;
  hipLaunchKernelGGL(k_sym_from_planes, dim3(nt * (nt + 1) / 2), dim3(256), 0, c->stream, lt.dLpart.p, sp.So, sp.Sd, (int64_t)Mp, lt.T1.p);
}

// G (in T3) -> slab 0 of krow: k_kuu_grad, or for D > MAXD its windows of WIDE_SLICE dimensions
// hk (a Matern latent, D <= MAXD): k_kuu_grad_matern, which recomputes K' from Z with the call's host lengthscales and variance
void launch_kuu_grad(zigp_ctx* c, Latent& lt, int D, double jitter, const HostLatent* hk = nullptr) {
  const int Mp = lt.Mp;
  if (hk && is_matern(hk->kind))
    hipLaunchKernelGGL(k_kuu_grad_matern, dim3(Mp), dim3(256), 0, c->stream, lt.T3.p, lt.Kuu.p, jitter, lt.Z.p, lt.M, make_hyp(hk->ell, hk->var, D), hk->kind,
                       (int64_t)Mp, lt.krow.p);
  else if (D > MAXD)
    hipLaunchKernelGGL(k_kuu_grad_wide, dim3(Mp, ceil_div(D, WIDE_SLICE)), dim3(256), 0, c->stream, lt.T3.p, lt.Kuu.p, jitter, lt.Z.p, lt.M, D, (int64_t)Mp,
                       lt.krow.p);
  else hipLaunchKernelGGL(k_kuu_grad, dim3(Mp), dim3(256), 0, c->stream, lt.T3.p, lt.Kuu.p, jitter, lt.Z.p, lt.M, D, (int64_t)Mp, lt.krow.p);
}

// Taps of the M x M reverse stage (zigp_test_mxm_backward): tap(id, buffer) is called right after the launch that produced the value, before
// its buffer is reused; ids are ZIGP_MXM_TAP_* (include/zigp_diag.h).  A call of the library passes none: no launch is added or moved.
using MxmTap = std::function<int(int, const double*)>;
#define ZIGP_TAP(id, buf) do { if (tap) ZIGP_TRY(tap(id, buf)); } while (0)

// ---- M x M backward of one latent: G = dELBO/dKuu (symmetric) -> krow accumulators.  Every parametrisation runs the same head (the rank-1
// seeds and C1) and the same tail (dL -> Phi -> Q W -> S = W^T (Q W)); between them each has its own way to R, the matrix part of dL. ----
// Head: the rank-1 seeds from K gm (accumulated by k_kgrad): A1 gm = W (K gm) and, unwhitened, A2 gm = du = W^T (A1 gm); then C1 -> T1
int mxm_backward_head(zigp_ctx* c, Latent& lt, int D, Param par, const MxmTap& tap) {
  const int Mp = lt.Mp;
  double* kgm = lt.vec.p + 3 * Mp + 8;
  hipLaunchKernelGGL(k_gather, dim3(ceil_div(Mp, 256)), dim3(256), 0, c->stream, lt.krow.p, 2 + 2 * D, 1 + 2 * D, Mp, KG_SPLIT,
                     (int64_t)Mp * (2 + 2 * D), kgm);
  hipLaunchKernelGGL(k_gemv_rows, dim3(Mp), dim3(256), 0, c->stream, lt.W.p, kgm, (int64_t)Mp, lt.a1gm.p);
  if (!is_white(par)) hipLaunchKernelGGL(k_gemv_cols, dim3(Mp / 64), dim3(64, COL_LANES), 0, c->stream, lt.W.p, lt.a1gm.p, (int64_t)Mp, lt.du.p);
  latent_sym_from_planes(c, lt);
  ZIGP_TAP(ZIGP_MXM_TAP_C1, lt.T1.p);
  return 0;
}
// Diag: R = W^T V (lower part) -> T2 with V = T C1 + C1 T - C1, T = (W diag(s^2)) W^T; on the way dsq = diag(A2 G A2^T) = diag(W^T C1 W)
int mxm_backward_r_diag(zigp_ctx* c, Latent& lt, const MxmTap& tap) {
  const int Mp = lt.Mp, nb = Mp / BM, gridmm = ceil_div((int64_t)Mp * Mp, 256);
  // Y = C1 W -> T3 ; dsq[m] = sum_k W[k][m] Y[k][m]
  ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::Y, nb, lt.T1.p, lt.W.p, lt.T3.p, Mp, SK_STORE, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_Y, lt.T3.p);
  hipLaunchKernelGGL(k_coldot, dim3(Mp / 64), dim3(64, COL_LANES), 0, c->stream, lt.W.p, lt.T3.p, (int64_t)Mp, lt.dsq.p);
  // T -> T2
  ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_KCONTIG>(c, lt.sk, SkRule::TT, nb, lt.Wp.p, lt.W.p, lt.T2.p, Mp, SK_STORE, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_T, lt.T2.p);
  // U = T C1 -> T3 ; V = U + U^T - C1 -> G
  ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::FULL, nb, lt.T2.p, lt.T1.p, lt.T3.p, Mp, SK_STORE, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_U, lt.T3.p);
  hipLaunchKernelGGL(k_uut_minus, dim3(gridmm), dim3(256), 0, c->stream, lt.T3.p, lt.T1.p, (int64_t)Mp, lt.G.p);
  ZIGP_TAP(ZIGP_MXM_TAP_V, lt.G.p);
  ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::R, nb, lt.W.p, lt.G.p, lt.T2.p, Mp, SK_STORE, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_R, lt.T2.p);
  return 0;
}
// White, WhiteFull.  The single triangular solve A = W K leaves  dL = -tril(W^T dA A^T)  with  dA = u gm^T + 2 D A G, i.e.
//   dL = -tril(alpha (A gm)^T + 2 (W^T D) C1),   C1 = A G A^T,  alpha = W^T u,
// so ONE split-K product R = (W^T D) C1 (lower part) -> T2 replaces the T / U / V / Y chain; the factor image D W is in Wp (latents_forward).
// du's data part is A gm = W (K gm), ds's is diag(C1); k_dense_pack adds the KL parts from Latent::wh.
// WhiteFull: ds becomes dLq (latent_qfull_dlq, which also carries the KL part) and the left factor is R = W^T (T - I), dense: its image
// R^T is in Rt and every k block contributes to the lower tiles.
int mxm_backward_r_white(zigp_ctx* c, Latent& lt, Param par, bool with_kl, const MxmTap& tap) {
  const int Mp = lt.Mp, nb = Mp / BM;
  if (is_full(par)) {
    ZIGP_TRY(latent_qfull_dlq(c, lt, true, with_kl));
    ZIGP_TAP(ZIGP_MXM_TAP_Y, lt.T3.p);      // Y = C1 Lq
    ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::RFULL, nb, lt.Rt.p, lt.T1.p, lt.T2.p, Mp, SK_STORE, 1.0)));
  } else {
    hipLaunchKernelGGL(k_diag, dim3(ceil_div(Mp, 256)), dim3(256), 0, c->stream, lt.T1.p, (int64_t)Mp, lt.dsq.p);
    ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::R, nb, lt.Wp.p, lt.T1.p, lt.T2.p, Mp, SK_STORE, 1.0)));
  }
  ZIGP_TAP(ZIGP_MXM_TAP_R, lt.T2.p);
  return 0;
}
// Tail: dL = -tril(alpha (A1 gm)^T + r1 r2^T + 2 R) -> T1 ; Q = Phi(L^T dL) -> T2 (upper tiles are not computed) ; T = Q W -> T3 (lower) ;
// S = W^T T -> T1.  r1, r2: the second rank-1 term, which differs by parametrisation (latent_mxm_backward).
int mxm_backward_tail(zigp_ctx* c, Latent& lt, const double* r1, const double* r2, const MxmTap& tap) {
  const int Mp = lt.Mp, nb = Mp / BM;
  hipLaunchKernelGGL(k_dl_assemble, dim3(ceil_div((int64_t)Mp * Mp, 256)), dim3(256), 0, c->stream, lt.T2.p, (int64_t)Mp, lt.vec.p + Mp, lt.a1gm.p, r1,
                     r2, lt.T1.p);
  ZIGP_TAP(ZIGP_MXM_TAP_DL, lt.T1.p);
  ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::R, nb, lt.L.p, lt.T1.p, lt.T2.p, Mp, SK_PHI, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_Q, lt.T2.p);
  ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::T, nb, lt.T2.p, lt.W.p, lt.T3.p, Mp, SK_STORE, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_QW, lt.T3.p);
  ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::S, nb, lt.W.p, lt.T3.p, lt.T1.p, Mp, SK_STORE, 1.0)));
  ZIGP_TAP(ZIGP_MXM_TAP_S, lt.T1.p);
  return 0;
}
int latent_mxm_backward(zigp_ctx* c, Latent& lt, int D, double jitter, Param par, bool with_data, bool with_kl, const MxmTap& tap,
                        const HostLatent* hk = nullptr) {
  const int Mp = lt.Mp, nb = Mp / BM;
  const size_t mm = (size_t)Mp * Mp;
  ZIGP_ENSURE(c, lt.T1, mm); ZIGP_ENSURE(c, lt.T2, mm); ZIGP_ENSURE(c, lt.T3, mm);
  if (!is_white(par)) ZIGP_ENSURE(c, lt.G, mm);
  const int gridmm = ceil_div((int64_t)mm, 256);
  if (with_data) {
    ZIGP_TRY(mxm_backward_head(c, lt, D, par, tap));
    if (is_white(par)) ZIGP_TRY(mxm_backward_r_white(c, lt, par, with_kl, tap));
    else ZIGP_TRY(mxm_backward_r_diag(c, lt, tap));
    // unwhitened: (A2 gm) v^T; whitened: `du` is zeroed per call and never written, so du du^T switches the term off
    ZIGP_TRY(mxm_backward_tail(c, lt, lt.du.p, is_white(par) ? lt.du.p : lt.vec.p, tap));
  } else if (is_full(par)) ZIGP_TRY(latent_qfull_dlq(c, lt, false, with_kl));      // dLq's KL part needs no rows
  if (is_white(par)) {
    // G = sym(S) -> T3 : no KL part (the white KL does not depend on Kuu)
    hipLaunchKernelGGL(k_sym_combine, dim3(gridmm), dim3(256), 0, c->stream, lt.T1.p, lt.T1.p, lt.T1.p, lt.vec.p + Mp, with_data ? 1 : 0, 0,
                       (int64_t)Mp, lt.T3.p);
  } else {
    double* P = lt.P_ready ? lt.P.p : lt.T2.p; double* PSP = lt.G.p;
    if (with_kl) {
      // P = W^T W -> T2   (a gradient step has it from the forward stage: latents_forward)
      if (!lt.P_ready) {
        ZIGP_TRY((run_gemm_sk<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::S, nb, lt.W.p, lt.W.p, lt.T2.p, Mp, SK_STORE, 1.0)));
        ZIGP_TAP(ZIGP_MXM_TAP_P, lt.T2.p);
      }
      // Ps = diag(s2) P -> T3 ; PSP = P Ps -> G
      hipLaunchKernelGGL(k_rowscale, dim3(gridmm), dim3(256), 0, c->stream, P, lt.s2.p, (int64_t)Mp, lt.T3.p);
      ZIGP_TRY((run_gemm_sk<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.sk, SkRule::FULL, nb, P, lt.T3.p, lt.G.p, Mp, SK_STORE, 1.0)));
      ZIGP_TAP(ZIGP_MXM_TAP_PSP, lt.G.p);
    }
    // G = sym(S) - dKL/dKuu -> T3 (T3 free again)
    hipLaunchKernelGGL(k_sym_combine, dim3(gridmm), dim3(256), 0, c->stream, lt.T1.p, P, PSP, lt.vec.p + Mp, with_data ? 1 : 0, with_kl ? 1 : 0,
                       (int64_t)Mp, lt.T3.p);
  }
  launch_kuu_grad(c, lt, D, jitter, hk);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

int validate_params(zigp_ctx* c, const zigp_params* p) {
  if (!p) return fail_arg(c, "params is NULL");
  if (p->Mf <= 0 || p->Mg <= 0) return fail_arg(c, "Mf and Mg must be positive");
  if (p->D <= 0 || p->D > ZIGP_MAX_D) return fail_arg(c, "D must be in [1, " ZIGP_MAX_D_STR "] (ZIGP_MAX_D)");
  if (p->D > MAXD) {
    std::string who;
    if (matern_latent(c, who))
      return fail_arg(c, ("a " + who + " (zigp_set_kernel) and D = " + std::to_string(p->D) + ": the Matern kernels cover D in [1, 8] (the wide kernels are RBF only)").c_str());
  }
  if (p->D > MAXD && c->mean_on)
    for (int d = 0; d < MAXD; ++d)
      if (c->mean_a[d] != 0.0) return fail_arg(c, "a Linear mean function is set and D > 8: Linear covers D in [1, 8] (Zero and Constant work at every D)");
  if (!p->Zf || !p->Zg || !p->u_fm || !p->u_gm || !p->u_fs_sqrt || !p->u_gs_sqrt || !p->ell_f || !p->ell_g)
    return fail_arg(c, "NULL pointer in params");
  if (!(p->var_f > 0) || !(p->var_g > 0) || !(p->noise > 0)) return fail_arg(c, "variances must be positive");
  for (int d = 0; d < p->D; ++d)
    if (!(p->ell_f[d] > 0) || !(p->ell_g[d] > 0)) return fail_arg(c, "lengthscales must be positive");
  if (c->q_full) {     // (M, M) lower-triangular factors; a negative diagonal entry is legal (the KL takes the log of the square), a zero one is not
    if (!c->whiten) return fail_arg(c, "zigp_set_q_full is on while whitening is off: the full-covariance q(u) exists for the whitened model only (zigp_set_whiten)");
    for (int m = 0; m < p->Mf; ++m)
      if (!(p->u_fs_sqrt[(size_t)m * p->Mf + m] != 0)) return fail_arg(c, "u_fs_sqrt has a zero (or NaN) diagonal entry (full q_sqrt, zigp_set_q_full)");
    for (int m = 0; m < p->Mg; ++m)
      if (!(p->u_gs_sqrt[(size_t)m * p->Mg + m] != 0)) return fail_arg(c, "u_gs_sqrt has a zero (or NaN) diagonal entry (full q_sqrt, zigp_set_q_full)");
    return 0;
  }
  for (int m = 0; m < p->Mf; ++m)
    if (!(p->u_fs_sqrt[m] > 0)) return fail_arg(c, "u_fs_sqrt must be positive (diagonal q_sqrt, transforms.positive)");
  for (int m = 0; m < p->Mg; ++m)
    if (!(p->u_gs_sqrt[m] > 0)) return fail_arg(c, "u_gs_sqrt must be positive (diagonal q_sqrt, transforms.positive)");
  return 0;
}

// ---- one call of the dense path (zigp_elbo / zigp_predict), in four stages: MxM forward, chunk loop, MxM backward, gather ----
struct DenseCall {
  const zigp_params* p; const double* dX; const double* dY; int64_t Nrows; int D;
  double jitter, scale, g_offset; int64_t row_begin, row_end; int include_kl; bool predict; double* d_out9;
  bool need_grad, has_rows;
  Param par = Param::Diag;      // the context's zigp_set_whiten / zigp_set_q_full at the time of the call (run_dense), or the fit loop's mode
  bool dlq_as_triangle = false; // packing choice of the fit loop, not a parametrisation: a WhiteFull step's dLq leaves as its lower triangle,
                                // M (M + 1) / 2 entries (k_pack_tril), not as the (M, M) block zigp_elbo returns
  HostLatent hl[2]; const double* ell_h[2];
  int64_t Nc = 0;         // rows per full chunk
  ChunkPlan plan[2];      // the full chunk and, if smaller, the last one (run_dense)
  int pw_blocks = 0;
  int* hinfo = nullptr;   // Cholesky status, staged with the other results
  bool prep_side = false; // buffers / zeroed accumulators / first Kuf panels were issued on the third stream (dense_mxm_forward)
  // a step of zigp_fit_steps: the parameter image and this hyperparameter block are on the device already (k_dense_fit_image), nothing is
  // staged, and a failed factorisation of latent h is left in d_info2[h] for the update kernel (p and hl carry the sizes only)
  const double* d_hyp = nullptr; int* d_info2 = nullptr;
  // zigp_head_elbo / zigp_head_predict: ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI -- the point-wise stage is k_pointwise_head, hl[1] is the
  // library's placeholder latent (head_placeholder) and its KL and gradient blocks are left out of the result (dense_gather); 0: OnOff
  int lik = 0;
  const double* hyp_rec(int h) const { return d_hyp ? d_hyp + h * DH_LAT : nullptr; }
};

// Parameters to the device, then the MxM forward of f on the main stream and of g on stream2 (dozens of small dependent launches each)
int dense_prepare_buffers(zigp_ctx* c, DenseCall& k);
int64_t dense_first_chunk_rows(const DenseCall& k) { return std::min<int64_t>(k.Nc, round_up(k.row_end - k.row_begin, 1024)); }
int dense_mxm_forward(zigp_ctx* c, DenseCall& k) {
  if (k.d_hyp) ZIGP_HIP(c, hipMemsetAsync(k.d_info2, 0, 2 * sizeof(int), c->stream));
  else {
    ZIGP_TRY(begin_staged_call(c));
    ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
    ZIGP_TRY(latents_upload(c, k.hl, k.D, k.par));
  }
  // The call's buffers, its zeroed accumulators and the first chunk's Kuf panels need the uploaded parameters only: third stream, under
  // the two factorisation chains (which are dependent launches of <= 36 workgroups).  Not while kernels are being timed (they run alone).
  k.prep_side = c->overlap == 1 && !c->prof_on;
  if (k.prep_side) {     // the main stream waits for ev_prep before the chunk loop (run_dense)
    ZIGP_TRY(fork_side(c, c->ev_prep_fork, c->stream3));
    OnStream on(c, c->stream3);
    ZIGP_TRY(dense_prepare_buffers(c, k));
    if (k.has_rows)
      for (int h = 0; h < 2; ++h)
        ZIGP_TRY(latent_chunk_kuf(c, c->lat[h], k.dX, k.Nrows, k.row_begin, dense_first_chunk_rows(k), k.D, k.ell_h[h], k.hyp_rec(h), k.hl[h].kind,
                                  k.need_grad));
    ZIGP_HIP(c, hipEventRecord(c->ev_prep, c->stream3));
  }
  {
    ProfScope ps(c, PC_MXM);     // wall time of the two concurrent chains: both events on the main stream, the second after the join
    ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
    ZIGP_TRY(latents_forward(c, k.hl, k.D, k.jitter, k.par, true, k.need_grad, k.d_hyp, k.d_info2));
    ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  }
  return k.d_hyp ? 0 : request_info(c, &k.hinfo);   // read after the final synchronisation
}

// Chunk size and per-call buffers.  The row range is cut into ceil(span / chunk) chunks of (nearly) equal size, a multiple of 1024, so
// that the last chunk is not a sliver whose GEMMs leave most of the 512 workgroup slots empty (N = 1e5, chunk 32768: 4 x 25600).
// Unless the caller fixed it (zigp_set_chunk), the chunk scales with 1 / M so that a launch keeps its ~2000 tiles (4 waves of the 512
// workgroup slots) and the panels their size: 32768 rows at M = 1024, 65536 at M = 512 (cfg2: 2 chunks instead of 4, 8.05 -> 7.6 ms)
int64_t auto_chunk_for(bool chunk_auto, int64_t chunk_set, int64_t Mp) {
  if (!chunk_auto) return chunk_set;
  return std::min<int64_t>(131072, std::max<int64_t>(32768, round_up(32768 * 1024 / std::max<int64_t>(Mp, 128), 1024)));
}
// Rows per pass for a row range of `span` rows.  A range of up to 131072 rows goes through in ONE pass unless the caller fixed the chunk: no
// chunk boundary (where the side stream's kgrads outlast the rank-N updates), one prologue / tail per product instead of two to four -- cfg2
// (1e5 rows, M = 512) 5.98 -> 5.81 ms, the 125 000-row shard of cfg3 23.4 -> 23.0 ms (tools/chunk_sweep.py, profiles/r04ao_chunk_sweep.log).
// The rule is bounded by the panels' bytes: a call holds 3 panels of 8 Mp span bytes per latent (K, A1, J'), and the bound budgets 4 of
// them against 9 GB -- deliberately conservative: one pass was measured only up to M = 1024 at 131072 rows.  Beyond that, and on long
// ranges, the M-scaled chunk applies (cfg3: 32768 rows 167.8 ms, 65536: 170.2, 131072: 169.2).
int64_t chunk_rows_for(bool chunk_auto, int64_t chunk_set, int64_t Mp, int64_t span) {
  int64_t chunk = auto_chunk_for(chunk_auto, chunk_set, Mp);
  if (chunk_auto && span > 0 && span <= 131072 && 4 * 2 * 8 * Mp * round_up(span, 1024) <= ((int64_t)9 << 30)) chunk = 131072;
  if (span <= 0) return 1024;
  const int64_t nchunks = (span + chunk - 1) / chunk;
  return std::max<int64_t>(1024, round_up((span + nchunks - 1) / nchunks, 1024));
}
int dense_prepare_buffers(zigp_ctx* c, DenseCall& k) {
  const int64_t Nc = k.Nc;
  const int D = k.D;
  k.pw_blocks = (int)(Nc / PW_PTS);
  ZIGP_ENSURE(c, c->pw_part, (size_t)k.pw_blocks * PW_ACC);
  ZeroRanges zr;               // the small accumulators of the call: one launch instead of a memset each
  zr.count = 0;
  static_assert(1 + 2 * 4 <= ZERO_RANGES_MAX, "one launch zeroes every small accumulator of a call");
  auto zero = [&](double* ptr, int64_t n) { zr.p[zr.count] = ptr; zr.n[zr.count] = n; ++zr.count; };
  zero(c->pw_part.p, (int64_t)k.pw_blocks * PW_ACC);
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const int Mp = lt.Mp;
    ZIGP_ENSURE(c, lt.gm, Nc); ZIGP_ENSURE(c, lt.gv, Nc);
    if (k.has_rows) {
      ZIGP_ENSURE(c, lt.K, (size_t)Mp * Nc);
      if (k.par != Param::White || k.need_grad) ZIGP_ENSURE(c, lt.A1, (size_t)Mp * Nc);     // a whitened (diagonal) value-only / predict pass stores no panel but K
      ZIGP_ENSURE(c, lt.part, (size_t)3 * (Mp / 32) * Nc);
      if (k.need_grad) ZIGP_ENSURE(c, lt.Jp, (size_t)Mp * Nc);
      // a Matern latent's gradient step: the derivative panel K', the fourth of the four panels per latent chunk_rows_for budgets
      if (k.need_grad && is_matern(k.hl[h].kind)) ZIGP_ENSURE(c, lt.Kd, (size_t)Mp * Nc);
      if (k.need_grad && D > MAXD && !lt.kg_exact) ZIGP_TRY(ensure_kgrad_wide(c, lt, Nc));
    }
    if (k.need_grad) {
      ZIGP_ENSURE(c, lt.du, Mp); ZIGP_ENSURE(c, lt.dsq, Mp); ZIGP_ENSURE(c, lt.krow, (size_t)KG_SPLIT * Mp * (2 + 2 * D));
      const int S = syr_plan(Mp / BM).planes();
      ZIGP_ENSURE(c, lt.dLpart, (size_t)S * Mp * Mp);
      ZIGP_ENSURE(c, lt.a1gm, Mp);
      zero(lt.a1gm.p, Mp); zero(lt.du.p, Mp); zero(lt.dsq.p, Mp); zero(lt.krow.p, (int64_t)KG_SPLIT * Mp * (2 + 2 * D));
      if (k.has_rows) ZIGP_HIP(c, hipMemsetAsync(lt.dLpart.p, 0, sizeof(double) * S * Mp * Mp, c->stream));
    }
  }
  hipLaunchKernelGGL(k_zero_ranges, dim3(64), dim3(256), 0, c->stream, zr);      // at most 1 + 2 x 4 ranges
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

// point-wise stage of the chunk starting at row n0 (probit moments, expected log-likelihood, reverse pass to gm / gv)
PwArgs dense_pointwise_args(zigp_ctx* c, const DenseCall& k, int64_t n0, int64_t Nc) {
  PwArgs a;
  a.part_f = c->lat[0].part.p; a.part_g = c->lat[1].part.p; a.np_f = c->lat[0].Mp / 32; a.np_g = c->lat[1].Mp / 32;
  {
    constexpr int RW2 = Shape<WavesFor<LAY_MNCONTIG, LAY_MNCONTIG, false>::value>::RW, RW1 = RW2;
    static_assert(RW1 >= 32 && RW2 >= 32, "partial-row planes are allocated for 32-row wave tiles");
    a.np1_f = c->lat[0].Mp / RW1; a.np2_f = c->lat[0].Mp / RW2; a.np1_g = c->lat[1].Mp / RW1; a.np2_g = c->lat[1].Mp / RW2;
  }
  a.Y = k.dY; a.n0 = n0; a.row_end = k.row_end; a.Nc = Nc;
  a.var_f = k.p->var_f; a.var_g = k.p->var_g; a.noise = k.p->noise; a.g_offset = k.g_offset; a.scale = k.scale;
  a.gm_f = k.need_grad ? c->lat[0].gm.p : nullptr; a.gv_f = c->lat[0].gv.p; a.gm_g = c->lat[1].gm.p; a.gv_g = c->lat[1].gv.p;
  a.X = k.dX; a.D = k.D; a.mean_on = c->mean_on ? 1 : 0; a.mean_b = c->mean_b;
  for (int d = 0; d < MAXD; ++d) a.mean_a[d] = (d < k.D) ? c->mean_a[d] : 0.0;
  a.acc = c->pw_part.p; a.out9 = k.d_out9 ? k.d_out9 - k.row_begin : nullptr; a.ld9 = k.row_end - k.row_begin;
  return a;
}
// k_pointwise<predict, plane-2 variance form>: the variance is var0 + (plane 2) instead of var0 - (plane 1) + (plane 2).  That form holds for
//   a gradient step   -- Diag, WhiteFull: plane 2 = sum_m K J' (the J' epilogue); a predict pass is never one
//   a fit-loop step   -- d_hyp: always a gradient step, through the overload that reads the device hyperparameter block
//   a White call      -- plane 2 = sum (s^2 - 1) A^2 in every mode (chunk_forward_white); a value-only pass has gm_f = NULL and writes no cotangents
// (a WhiteFull value-only / predict call is the unwhitened form: var0 - sum A^2 + sum B^2)
// lik != 0 (DenseCall::lik): the head's kernel on the planes of f, in the same three forms; a head call has no device hyperparameter block
static_assert(PWH_GAUSSIAN == ZIGP_LIK_GAUSSIAN && PWH_BERNOULLI == ZIGP_LIK_BERNOULLI, "the head kernel's LIK values are the ZIGP_LIK_* constants");
template <int LIK>
void pointwise_head_launch(zigp_ctx* c, const dim3& grid, const dim3& block, bool predict, bool plane2, const PwArgs& a) {
  if (predict && plane2) hipLaunchKernelGGL((k_pointwise_head<LIK, true, true>), grid, block, 0, c->stream, a);
  else if (predict) hipLaunchKernelGGL((k_pointwise_head<LIK, true, false>), grid, block, 0, c->stream, a);
  else if (plane2) hipLaunchKernelGGL((k_pointwise_head<LIK, false, true>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_pointwise_head<LIK, false, false>), grid, block, 0, c->stream, a);
}
int dense_pointwise_launch(zigp_ctx* c, Param par, bool predict, bool need_grad, const PwArgs& a, const double* d_hyp, int lik = 0) {
  ProfScope ps(c, PC_POINT);
  const dim3 grid((unsigned)(a.Nc / PW_PTS)), block(PW_THREADS);
  const bool plane2 = need_grad || d_hyp || par == Param::White;
  if (lik == ZIGP_LIK_GAUSSIAN) pointwise_head_launch<PWH_GAUSSIAN>(c, grid, block, predict, plane2, a);
  else if (lik == ZIGP_LIK_BERNOULLI) pointwise_head_launch<PWH_BERNOULLI>(c, grid, block, predict, plane2, a);
  else if (d_hyp) hipLaunchKernelGGL((k_pointwise<false, true>), grid, block, 0, c->stream, a, d_hyp);
  else if (predict && plane2) hipLaunchKernelGGL((k_pointwise<true, true>), grid, block, 0, c->stream, a);
  else if (predict) hipLaunchKernelGGL((k_pointwise<true, false>), grid, block, 0, c->stream, a);
  else if (plane2) hipLaunchKernelGGL((k_pointwise<false, true>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_pointwise<false, false>), grid, block, 0, c->stream, a);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
int dense_pointwise(zigp_ctx* c, const DenseCall& k, int64_t n0, int64_t Nc) {
  return dense_pointwise_launch(c, k.par, k.predict, k.need_grad, dense_pointwise_args(c, k, n0, Nc), k.d_hyp, k.lik);
}

// ---- chunk loop.  The MFMA-bound GEMMs stay on the main stream; with zigp_set_overlap(1) the HBM-bound kernels of a chunk -- the two
// Kuf-cotangent reductions and the two Kuf panels of the NEXT chunk -- run on the side stream underneath the chunk's two SYRKs:
//   main:  [wait side]  A1 (f|g)  J' (f|g)  point-wise  (record)  SYRK f  SYRK g
//   side:                                              (wait)    kgrad f  kgrad g  Kuf f'  Kuf g'  (record)
// K is read by A1 and by J''s epilogue (sum K J'), and by kgrad; the fork comes after both, so the next chunk's panels never overwrite a
// K that J' still reads.  J' / gm are read only by kgrad: the next chunk's GEMMs wait for the side stream, nothing else is shared.
// A chunk whose kernels are being timed (profiling samples every prof_every-th chunk) runs everything on the main stream, so the
// per-kernel durations bench.py reports are those of kernels running alone.
int dense_chunk_loop(zigp_ctx* c, const DenseCall& k) {
  if (!k.has_rows) return 0;
  const int64_t Nc_full = k.Nc, row_begin = k.row_begin, row_end = k.row_end;
  const int D = k.D;
  auto chunk_rows = [&](int64_t n0) { return std::min<int64_t>(Nc_full, round_up(row_end - n0, 1024)); };
  auto sampled = [&](int64_t n0) {   // kernel timing (HIP events) covers FULL chunks only, so the averages describe full-size launches
    if (!c->prof_on) return false;
    if (c->prof_every <= 1 || row_end - row_begin <= Nc_full) return true;   // every launch, the partial last chunk included
    return chunk_rows(n0) == Nc_full && (((n0 - row_begin) / Nc_full) % c->prof_every) == 0;
  };
  auto kuf = [&](int64_t n0) -> int {     // Kuf panels of both latents for the chunk at row n0
    for (int h = 0; h < 2; ++h)
      ZIGP_TRY(latent_chunk_kuf(c, c->lat[h], k.dX, k.Nrows, n0, chunk_rows(n0), D, k.ell_h[h], k.hyp_rec(h), k.hl[h].kind, k.need_grad));
    return 0;
  };
  auto kgrad = [&](int64_t n0, int64_t Nc) -> int {
    const ChunkPlan& pl = k.plan[Nc == k.plan[0].Nc ? 0 : 1];
    for (int h = 0; h < 2; ++h) ZIGP_TRY(latent_chunk_kgrad(c, c->lat[h], k.dX, k.Nrows, n0, Nc, D, k.ell_h[h], pl.lat[h].mom, k.hl[h].kind));
    return 0;
  };
  // Side-stream section: stream2 forks from the main stream, runs `work` and records ev_join, which the main stream waits on
  // (wait_side) before the next A1 -- or before panels it builds itself, or at the end of the loop.
  bool side_busy = false;
  auto on_side = [&](auto work) -> int {
    ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
    OnStream on(c, c->stream2);
    ZIGP_TRY(work());
    ZIGP_HIP(c, hipEventRecord(c->ev_join, c->stream2));
    side_busy = true;
    return 0;
  };
  auto wait_side = [&]() -> int {
    if (side_busy) ZIGP_HIP(c, hipStreamWaitEvent(c->stream_main, c->ev_join, 0));
    side_busy = false;
    return 0;
  };
  c->prof_skip = c->prof_on && !sampled(row_begin);
  if (!k.prep_side) ZIGP_TRY(kuf(row_begin));     // (otherwise built on the third stream under the M x M forward: dense_mxm_forward)
  for (int64_t n0 = row_begin; n0 < row_end; n0 += Nc_full) {
    const int64_t Nc = chunk_rows(n0);   // the last (partial) chunk shrinks to the next multiple of 1024 rows
    const int64_t n1 = n0 + Nc_full;
    const bool has_next = n1 < row_end;
    const bool timed = sampled(n0), timed_next = has_next && sampled(n1);
    c->prof_skip = c->prof_on && !timed;
    // A1 of this chunk needs the Kuf panels the side stream built behind the previous chunk's kgrads (which read J' and gm)
    ZIGP_TRY(wait_side());
    // value-only ELBO and predict (r6): there are no rank-N updates to hide the next chunk's Kuf panels under, but K has ONE reader there
    // -- A1 -- so the side stream builds the next panels right behind this chunk's A1, beside its A2 product and point-wise stage
    // (cfg3 value-only: the 4 ms of panel building per pass were serial on the main stream)
    const bool kuf_fwd_side = c->overlap == 1 && c->fwd_kuf_side && !k.need_grad && has_next && !timed && !timed_next;
    std::function<int()> after_a1;
    if (kuf_fwd_side) after_a1 = [&] { return on_side([&] { return kuf(n1); }); };
    const ChunkPlan& pl = k.plan[Nc == k.plan[0].Nc ? 0 : 1];
    if (k.par == Param::White) {     // A (f|g), point-wise (it needs the A launch only), then J' (f|g) of a gradient step
      ZIGP_TRY(chunk_forward_white(c, pl, k.need_grad, false, after_a1));
      ZIGP_TRY(dense_pointwise(c, k, n0, Nc));
      if (k.need_grad) ZIGP_TRY(chunk_forward_white(c, pl, true, true));
    } else {     // Diag: A1 (f|g), then A2 (sums only) or J'; WhiteFull: the same order -- A, then B = Lq^T A (sums only) or J' = R A
      ZIGP_TRY(chunk_forward(c, pl, k.par, k.need_grad, after_a1));
      // the point-wise stage of a gradient step needs the J' launch's sums (it rode inside the J' launch while the variance came from A2:
      // r5, profiles/r05t_ab_fuse_pointwise.log), so it is a launch of its own after it
      ZIGP_TRY(dense_pointwise(c, k, n0, Nc));
    }
    // side work of this chunk: its kgrads and the next chunk's Kuf panels (gradient mode only: without the SYRKs there is
    // nothing on the main stream to hide them under)
    const bool kgrad_side = c->overlap == 1 && k.need_grad && !timed;
    const bool kuf_side = kgrad_side && has_next && !timed_next;
    if (kgrad_side)
      ZIGP_TRY(on_side([&]() -> int {
        // (the next chunk's panels BEFORE this chunk's kgrads was measured and dropped: cfg2 +0.1 ms, HISTORY.md section 5 r4)
        ZIGP_TRY(kgrad(n0, Nc));
        return kuf_side ? kuf(n1) : 0;
      }));
    if (k.need_grad) {
      if (!kgrad_side) ZIGP_TRY(kgrad(n0, Nc));
      for (int h = 0; h < 2; ++h) ZIGP_TRY(latent_chunk_syrk(c, pl, h));
    }
    if (has_next && !kuf_side && !kuf_fwd_side) {   // a timed next chunk gets its panels from the main stream, with the side stream drained
      ZIGP_TRY(wait_side());
      c->prof_skip = c->prof_on && !timed_next;
      ZIGP_TRY(kuf(n1));
    }
  }
  return wait_side();
}

// The call's result vector (layout: k_dense_pack) is assembled on the device, summed over the ranks of a data-parallel run where it
// lies (zigp_comm_init; no-op otherwise), downloaded once and unpacked: the call's single synchronisation.
int dense_pack(zigp_ctx* c, const DenseCall& k, DensePackArgs& a, size_t& n) {
  const int D = k.D;
  n = DP_HDR;
  memset(&a, 0, sizeof(a));
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    DensePackLat& L = a.lat[h];
    L.krow = lt.krow.p; L.du = lt.du.p; L.dsq = lt.dsq.p; L.vec = lt.vec.p; L.s = lt.s.p; L.ell = lt.ell.p;
    // whitened: du's data part is A gm, the KL parts and the KL value come from the whitened vectors (k_kl_white keeps vec's layout)
    if (is_white(k.par)) { L.du = lt.a1gm.p; L.vec = lt.wh.p; }
    L.M = lt.M; L.Mp = lt.Mp; L.var = lt.var; L.out_off = (int64_t)n; L.q_full = is_full(k.par) ? 1 : 0;
    L.ns = !is_full(k.par) ? (int64_t)lt.M : k.dlq_as_triangle ? (int64_t)lt.M * (lt.M + 1) / 2 : (int64_t)lt.M * lt.M;
    if (k.need_grad) n += (size_t)lt.M * D + (size_t)lt.M + (size_t)L.ns + D;
  }
  a.pw = c->pw_part.p; a.pw_blocks = k.pw_blocks; a.D = D; a.need_grad = k.need_grad ? 1 : 0; a.include_kl = k.include_kl ? 1 : 0;
  a.mean_on = c->mean_on ? 1 : 0;
  ZIGP_ENSURE(c, c->packed, n);
  a.out = c->packed.p;
  if (k.d_hyp) hipLaunchKernelGGL(k_dense_pack<const double*>, dim3(2), dim3(256), 0, c->stream, a, k.d_hyp);
  else hipLaunchKernelGGL(k_dense_pack<>, dim3(2), dim3(256), 0, c->stream, a);
  if (k.need_grad && is_full(k.par))
    for (int h = 0; h < 2; ++h) {     // the (M, M) blocks, behind du
      const Latent& lt = c->lat[h];
      double* os = a.out + a.lat[h].out_off + (int64_t)lt.M * D + lt.M;
      const dim3 grid(ceil_div((int64_t)lt.M * lt.M, 256));
      if (k.dlq_as_triangle) hipLaunchKernelGGL(k_pack_tril, grid, dim3(256), 0, c->stream, lt.dLq.p, lt.M, (int64_t)lt.Mp, os);
      else hipLaunchKernelGGL(k_pack_square, grid, dim3(256), 0, c->stream, lt.dLq.p, lt.M, (int64_t)lt.Mp, os);
    }
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
int dense_gather(zigp_ctx* c, DenseCall& k, double* elbo_data, double* kl, zigp_grads* grads) {
  const int D = k.D;
  size_t n = 0;
  DensePackArgs a;
  ZIGP_TRY(dense_pack(c, k, a, n));
  ZIGP_TRY(comm_allreduce(c, c->packed.p, n));
  double* hv = nullptr;
  ZIGP_TRY(download(c, c->packed.p, n, &hv));
  // a head call: KL_f as the M x M forward left it (where k_dense_pack and zigp_prior_kl read it), not the packed sum with the placeholder's
  double* hkl_f = nullptr;
  if (k.lik) ZIGP_TRY(download(c, (is_white(k.par) ? c->lat[0].wh.p : c->lat[0].vec.p) + 3 * c->lat[0].Mp, 1, &hkl_f));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  ZIGP_TRY(info_result(c, k.hinfo, "Kuu"));
  if (elbo_data) *elbo_data = hv[0];
  if (kl) *kl = !k.lik ? hv[1] : k.include_kl ? *hkl_f : 0.0;
  c->mean_db = hv[5];
  for (int d = 0; d < MAXD; ++d) c->mean_da[d] = hv[6 + d];
  if (k.need_grad) {
    double* gZ[2] = {grads->Zf, grads->Zg};
    double* gu[2] = {grads->u_fm, grads->u_gm};
    double* gs[2] = {grads->u_fs_sqrt, grads->u_gs_sqrt};
    double* gl[2] = {grads->ell_f, grads->ell_g};
    for (int h = 0; h < (k.lik ? 1 : 2); ++h) {     // (a head call: the placeholder's blocks stay where they are)
      const size_t M = (size_t)c->lat[h].M;
      const double* o = hv + a.lat[h].out_off;
      if (gZ[h]) memcpy(gZ[h], o, sizeof(double) * M * D);
      if (gu[h]) memcpy(gu[h], o + M * D, sizeof(double) * M);
      const size_t ns = is_full(k.par) ? M * M : M;
      if (gs[h]) memcpy(gs[h], o + M * D + M, sizeof(double) * ns);
      if (gl[h]) memcpy(gl[h], o + M * D + M + ns, sizeof(double) * D);
    }
    grads->var_f = hv[2]; grads->noise = hv[4];
    if (!k.lik) grads->var_g = hv[3];
  }
  return 0;
}

// Chunk size of the call and every tile list of its chunk loop, uploaded before the call enqueues anything
int dense_plan(zigp_ctx* c, DenseCall& k) {
  const int M[2] = {k.hl[0].M, k.hl[1].M};
  const int64_t span = k.has_rows ? k.row_end - k.row_begin : 0;
  k.Nc = chunk_rows_for(c->chunk_auto, c->chunk, round_up(std::max(M[0], M[1]), BM), span);
  if (k.has_rows) {
    const int64_t last = std::min<int64_t>(k.Nc, round_up(span - (span - 1) / k.Nc * k.Nc, 1024));
    k.plan[0] = chunk_plan(M, k.Nc, k.par, k.need_grad, c->trmm_tail, k.D > MAXD);
    ZIGP_TRY(upload_plan(c, k.plan[0]));
    if (last != k.Nc) { k.plan[1] = chunk_plan(M, last, k.par, k.need_grad, c->trmm_tail, k.D > MAXD); ZIGP_TRY(upload_plan(c, k.plan[1])); }
  }
  return 0;
}
// The launches of one call up to its result vector: M x M forward, chunk loop, M x M backward (gradient steps).  zigp_elbo / zigp_predict
// run it once (run_dense), zigp_fit_steps once per iteration, on the same streams and events.
int dense_step(zigp_ctx* c, DenseCall& k) {
  ZIGP_TRY(dense_mxm_forward(c, k));
  if (k.prep_side) ZIGP_HIP(c, hipStreamWaitEvent(c->stream_main, c->ev_prep, 0));
  else ZIGP_TRY(dense_prepare_buffers(c, k));
  const int rc = dense_chunk_loop(c, k);
  c->prof_skip = false;   // the loop sets it for the chunks it does not time; cleared on every exit path
  ZIGP_TRY(rc);
  if (k.need_grad) {
    ProfScope ps(c, PC_MXM);     // wall time of the two concurrent chains, as in the forward: both events on the main stream, the second after the join
    ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
    for (int h = 0; h < 2; ++h) {
      OnStream on(c, h == 0 ? c->stream_main : c->stream2);
      ZIGP_TRY(latent_mxm_backward(c, c->lat[h], k.D, k.jitter, k.par, k.has_rows, k.include_kl != 0, nullptr, &k.hl[h]));
    }
    ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  }
  return 0;
}

// shared driver for zigp_elbo / zigp_predict
// The placeholder latent a head call puts in DenseCall::hl[1] (include/zigp.h "heads on the dense path"): one inducing point at the origin,
// u = 0, s = 1 (the (1, 1) factor [1] of the full-covariance mode is the same double), ell = 1 in every dimension, var = 1, RBF
struct HeadPlaceholder {
  double Z[ZIGP_MAX_D], ell[ZIGP_MAX_D], u[1], s[1];
  HeadPlaceholder() { for (int d = 0; d < ZIGP_MAX_D; ++d) { Z[d] = 0.0; ell[d] = 1.0; } u[0] = 0.0; s[0] = 1.0; }
};
const HeadPlaceholder& head_placeholder() { static const HeadPlaceholder h; return h; }

int run_dense_lik(zigp_ctx* c, const zigp_params* p, int lik, const double* dX, const double* dY, int64_t Nrows, int D, double jitter,
                  double scale, double g_offset, int64_t row_begin, int64_t row_end, int include_kl, bool predict, double* d_out9,
                  double* elbo_data, double* kl, zigp_grads* grads);
int run_dense(zigp_ctx* c, const zigp_params* p, const double* dX, const double* dY, int64_t Nrows, int D, double jitter,
              double scale, double g_offset, int64_t row_begin, int64_t row_end, int include_kl, bool predict, double* d_out9,
              double* elbo_data, double* kl, zigp_grads* grads) {
  return run_dense_lik(c, p, 0, dX, dY, Nrows, D, jitter, scale, g_offset, row_begin, row_end, include_kl, predict, d_out9, elbo_data, kl, grads);
}
// lik != 0: a head call -- p is the library's copy of the caller's f half with the placeholder in the g fields (head_params)
int run_dense_lik(zigp_ctx* c, const zigp_params* p, int lik, const double* dX, const double* dY, int64_t Nrows, int D, double jitter,
                  double scale, double g_offset, int64_t row_begin, int64_t row_end, int include_kl, bool predict, double* d_out9,
                  double* elbo_data, double* kl, zigp_grads* grads) {
  DenseCall k;
  k.lik = lik;
  k.p = p; k.dX = dX; k.dY = dY; k.Nrows = Nrows; k.D = D; k.jitter = jitter; k.scale = scale; k.g_offset = g_offset;
  k.row_begin = row_begin; k.row_end = row_end; k.include_kl = include_kl; k.predict = predict; k.d_out9 = d_out9;
  k.need_grad = (grads != nullptr) && !predict;
  k.has_rows = row_end > row_begin;
  k.par = param_of(c);
  k.hl[0] = HostLatent{p->Mf, p->Zf, p->u_fm, p->u_fs_sqrt, p->ell_f, p->var_f, c->kern[0]};
  k.hl[1] = HostLatent{p->Mg, p->Zg, p->u_gm, p->u_gs_sqrt, p->ell_g, p->var_g, lik ? (int)ZIGP_KERN_RBF : c->kern[1]};
  k.ell_h[0] = p->ell_f; k.ell_h[1] = p->ell_g;
  ZIGP_TRY(dense_plan(c, k));
  ZIGP_TRY(dense_step(c, k));
  if (predict) { ZIGP_HIP(c, hipStreamSynchronize(c->stream)); prof_collect(c); return info_result(c, k.hinfo, "Kuu"); }
  return dense_gather(c, k, elbo_data, kl, grads);
}

}  // namespace

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

int zigp_create(zigp_ctx** out, int device_id) {
  if (!out) return ZIGP_EARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZIGP_EHIP;
  if (device_id < 0 || device_id >= ndev) return ZIGP_EARG;
  if (hipSetDevice(device_id) != hipSuccess) return ZIGP_EHIP;
  zigp_ctx* c = new (std::nothrow) zigp_ctx();
  if (!c) return ZIGP_EHIP;
  c->device = device_id;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return ZIGP_EHIP; }
  c->stream_main = c->stream;
  if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) { delete c; return ZIGP_EHIP; }
  if (hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking) != hipSuccess) { delete c; return ZIGP_EHIP; }
  if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_prep_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_prep, hipEventDisableTiming) != hipSuccess) { delete c; return ZIGP_EHIP; }
  if (hipMalloc((void**)&c->d_info, sizeof(int)) != hipSuccess) { delete c; return ZIGP_EHIP; }
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_potrf_diag<double>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(sizeof(double) * PB * PBLD)) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_potrf_diag<const double*>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(sizeof(double) * PB * PBLD)) != hipSuccess) { delete c; return ZIGP_EHIP; }
  if (const char* e = getenv("ZIGP_FWD_KUF_SIDE")) c->fwd_kuf_side = atoi(e) != 0;   // A/B switch (tools/ab_envs.sh); default on
  if (const char* e = getenv("ZIGP_TRMM_TAIL")) c->trmm_tail = atoi(e) != 0;      // A/B switch of the LPT tail (tools/ab_envs.sh); default on
  if (const char* e = getenv("ZIGP_COMM_TIMEOUT_S")) { const double v = atof(e); if (v > 0) c->comm_timeout_s = v; }
  *out = c;
  return ZIGP_OK;
}

// The context's destructor frees its buffers, then its events and streams (zigp_ctx.h); what must come first stays here.
int zigp_destroy(zigp_ctx* c) {
  if (!c) return ZIGP_EARG;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream_main);
  (void)hipStreamSynchronize(c->stream2);
  if (c->stream3) (void)hipStreamSynchronize(c->stream3);
  if (c->comm) { RcclApi* api = rccl_api(nullptr); if (api) (void)api->CommDestroy(static_cast<ncclComm_t>(c->comm)); c->comm = nullptr; }
  delete c;
  return ZIGP_OK;
}

const char* zigp_last_error(zigp_ctx* c) { return c ? c->err.c_str() : "null context"; }
int zigp_last_info(zigp_ctx* c) { return c ? c->info : 0; }

int zigp_set_overlap(zigp_ctx* c, int32_t on) {
  if (!c) return ZIGP_EARG;
  if (on < 0 || on > 1) return fail_arg(c, "zigp_set_overlap: mode must be 0 or 1");
  c->overlap = on;
  return ZIGP_OK;
}

int zigp_set_chunk(zigp_ctx* c, int64_t chunk_rows) {
  if (!c) return ZIGP_EARG;
  if (chunk_rows == 0) { c->chunk_auto = true; c->chunk = 32768; return ZIGP_OK; }   // back to the automatic rule
  if (chunk_rows < 1024 || chunk_rows % 1024 != 0) return fail_arg(c, "chunk must be a positive multiple of 1024 (or 0: automatic)");
  if (chunk_rows > (1 << 20)) return fail_arg(c, "chunk must be <= 1048576 rows (32-bit staging offsets; 3 panels (K, A1, J') of 8*M*chunk bytes per latent)");
  c->chunk = chunk_rows;
  c->chunk_auto = false;
  return ZIGP_OK;
}

int zigp_set_pivot_rtol(zigp_ctx* c, double rtol) {
  if (!c) return ZIGP_EARG;
  if (!(rtol >= 0) || !std::isfinite(rtol)) return fail_arg(c, "zigp_set_pivot_rtol: rtol must be finite and >= 0");
  c->pivot_rtol = rtol;
  return ZIGP_OK;
}

int64_t zigp_get_chunk(zigp_ctx* c, int32_t M) {
  if (!c || M <= 0) return ZIGP_EARG;
  return auto_chunk_for(c->chunk_auto, c->chunk, round_up(M, BM));
}

int64_t zigp_get_chunk_rows(zigp_ctx* c, int32_t M, int64_t span) {
  if (!c || M <= 0 || span < 0) return ZIGP_EARG;
  return chunk_rows_for(c->chunk_auto, c->chunk, round_up(M, BM), span);
}

static_assert(MAXD == 8, "zigp_ctx::mean_a / mean_da hold MAXD entries");

int zigp_set_mean_function(zigp_ctx* c, const double* a, int32_t D, double b) {
  if (!c) return ZIGP_EARG;
  if (D < -1 || D > MAXD || (D > 0 && !a)) return fail_arg(c, "zigp_set_mean_function: need -1 <= D <= 8 and a[D] (a Linear mean function covers D in [1, 8]; Zero and Constant work at every D)");
  if (D < 0) {   // Zero: no mean function, nothing to differentiate
    for (int d = 0; d < MAXD; ++d) c->mean_a[d] = 0.0;
    c->mean_b = 0.0; c->mean_on = false;
    return ZIGP_OK;
  }
  if (!std::isfinite(b)) return fail_arg(c, "zigp_set_mean_function: b must be finite");
  for (int d = 0; d < D; ++d)
    if (!std::isfinite(a[d])) return fail_arg(c, "zigp_set_mean_function: a must be finite");
  for (int d = 0; d < MAXD; ++d) c->mean_a[d] = (d < D) ? a[d] : 0.0;
  c->mean_b = b;
  c->mean_on = true;   // "enabled" is independent of the values: a Constant at exactly 0 still gets its gradient
  return ZIGP_OK;
}

int zigp_set_whiten(zigp_ctx* c, int32_t on) {
  if (!c) return ZIGP_EARG;
  if (on < 0 || on > 1) return fail_arg(c, "zigp_set_whiten: on must be 0 or 1");
  c->whiten = on != 0;
  return ZIGP_OK;
}
int zigp_get_whiten(zigp_ctx* c) { return c ? (c->whiten ? 1 : 0) : (int)ZIGP_EARG; }

int zigp_set_q_full(zigp_ctx* c, int32_t on) {
  if (!c) return ZIGP_EARG;
  if (on < 0 || on > 1) return fail_arg(c, "zigp_set_q_full: on must be 0 or 1");
  c->q_full = on != 0;
  return ZIGP_OK;
}
int zigp_get_q_full(zigp_ctx* c) { return c ? (c->q_full ? 1 : 0) : (int)ZIGP_EARG; }

int zigp_set_kernel(zigp_ctx* c, int32_t latent, int32_t kind) {
  if (!c) return ZIGP_EARG;
  if (latent < 0 || latent > 1) return fail_arg(c, "zigp_set_kernel: latent must be 0 (f) or 1 (g)");
  if (kind != ZIGP_KERN_RBF && kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52)
    return fail_arg(c, "zigp_set_kernel: unknown kernel kind (ZIGP_KERN_RBF, ZIGP_KERN_MATERN32, ZIGP_KERN_MATERN52)");
  c->kern[latent] = kind;
  if (!is_matern(kind)) {     // the derivative panel exists only while the latent is Matern (every call ends synchronised: nothing reads it now)
    (void)hipSetDevice(c->device);
    c->lat[latent].Kd.release();
  }
  return ZIGP_OK;
}
int zigp_get_kernel(zigp_ctx* c, int32_t latent) { return (c && latent >= 0 && latent <= 1) ? c->kern[latent] : (int)ZIGP_EARG; }

int zigp_get_mean_function_grad(zigp_ctx* c, double* da, int32_t D, double* db) {
  if (!c) return ZIGP_EARG;
  if (D < 0 || D > MAXD || (D > 0 && !da)) return fail_arg(c, "zigp_get_mean_function_grad: need 0 <= D <= 8 and da[D]");
  for (int d = 0; d < D; ++d) da[d] = c->mean_da[d];
  if (db) *db = c->mean_db;
  return ZIGP_OK;
}

int zigp_set_data(zigp_ctx* c, const double* X, const double* Y, int64_t N, int32_t D) {
  if (!c) return ZIGP_EARG;
  if (!X || !Y || N <= 0 || D <= 0 || D > ZIGP_MAX_D) return fail_arg(c, "zigp_set_data: bad arguments (need X, Y, N>0, 1<=D<=" ZIGP_MAX_D_STR ")");
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_ENSURE(c, c->ownX, (size_t)N * D);
  ZIGP_ENSURE(c, c->ownY, (size_t)N);
  ZIGP_HIP(c, hipMemcpyAsync(c->ownX.p, X, sizeof(double) * N * D, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(c->ownY.p, Y, sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  c->dX = c->ownX.p; c->dY = c->ownY.p; c->N = N; c->D = D;
  c->fullX = c->dX; c->fullY = c->dY; c->fullN = N;
  return ZIGP_OK;
}

int zigp_set_data_device(zigp_ctx* c, const double* dX, const double* dY, int64_t N, int32_t D) {
  if (!c) return ZIGP_EARG;
  if (!dX || !dY || N <= 0 || D <= 0 || D > ZIGP_MAX_D) return fail_arg(c, "zigp_set_data_device: bad arguments (need dX, dY, N>0, 1<=D<=" ZIGP_MAX_D_STR ")");
  c->dX = dX; c->dY = dY; c->N = N; c->D = D;
  c->fullX = dX; c->fullY = dY; c->fullN = N;
  return ZIGP_OK;
}

int zigp_select_rows(zigp_ctx* c, const int64_t* rows, int64_t n) {
  if (!c) return ZIGP_EARG;
  if (!c->fullX) return fail_arg(c, "zigp_select_rows: no data set (call zigp_set_data first)");
  if (n < 0 || (n > 0 && !rows)) return fail_arg(c, "zigp_select_rows: bad arguments");
  if (n == 0) { c->dX = c->fullX; c->dY = c->fullY; c->N = c->fullN; return ZIGP_OK; }   // back to the whole resident set
  for (int64_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= c->fullN) return fail_arg(c, "zigp_select_rows: row index out of range");
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(begin_staged_call(c));
  const int D = c->D;
  ZIGP_ENSURE(c, c->selX, (size_t)n * D); ZIGP_ENSURE(c, c->selY, (size_t)n); ZIGP_ENSURE(c, c->selIdx, (size_t)n);
  int64_t* h = (int64_t*)c->pinned.alloc(sizeof(int64_t) * n);
  if (!h) { c->err = "hipHostMalloc failed for the staging arena"; return ZIGP_EHIP; }
  memcpy(h, rows, sizeof(int64_t) * n);
  ZIGP_HIP(c, hipMemcpyAsync(c->selIdx.p, h, sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_gather_rows, dim3(ceil_div(n * (D + 1), 256)), dim3(256), 0, c->stream, c->fullX, c->fullY,
                     reinterpret_cast<const int64_t*>(c->selIdx.p), n, D, c->selX.p, c->selY.p);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));   // the staged index block may be reused by the next call
  c->dX = c->selX.p; c->dY = c->selY.p; c->N = n;
  return ZIGP_OK;
}

int zigp_elbo(zigp_ctx* c, const zigp_params* p, double jitter, double scale, double g_offset, int64_t row_begin, int64_t row_end,
              int32_t include_kl, double* elbo_data, double* kl, zigp_grads* grads) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  if (!c->dX) return fail_arg(c, "zigp_elbo: no data set (call zigp_set_data first)");
  if (p->D != c->D) return fail_arg(c, "zigp_elbo: params.D differs from the data's D");
  if (row_begin < 0 || row_end > c->N || row_begin > row_end) return fail_arg(c, "zigp_elbo: bad row range");
  if (!(jitter >= 0)) return fail_arg(c, "zigp_elbo: jitter must be >= 0");
  ZIGP_HIP(c, hipSetDevice(c->device));
  return run_dense(c, p, c->dX, c->dY, c->N, c->D, jitter, scale, g_offset, row_begin, row_end, include_kl, false, nullptr, elbo_data, kl,
                   grads);
}

// ---- the dense fit loop on the device (include/zigp.h) ----
// Host side of one call: everything is planned, sized and uploaded before the first step is enqueued (tile lists: dense_plan; the state,
// the moments and the row indices: one staged copy each); a step is k_gather_rows (minibatch) + dense_step + k_dense_pack +
// k_dense_fit_update + k_dense_fit_image on the call's main stream, its side work forked from and joined into it exactly as in zigp_elbo.
// The first step sizes the per-call buffers and fills the tile cache of the M x M stage; from the second step on nothing allocates, copies
// synchronously or synchronises until the one download at the end.
static_assert(DFIT_BLOCKS == ZIGP_DENSE_FIT_BLOCKS, "block order of include/zigp.h");
}  // extern "C"
namespace {
// One loop for the three parametrisations (include/zigp.h ZIGP_FIT_*).  `mode` decides the layout of blocks 4 and 5, the image kernels and
// DenseCall::par, i.e. which chunk lists dense_plan plans and which launches dense_step makes; `legacy` is zigp_fit_steps, which
// refuses while the context's own whiten / q_full flags are on -- zigp_fit_steps_mode neither reads nor changes them.
// State of the tapped loop: the caller's packed vectors and status ints on the device, and the snapshots x | m | v | image | H | Lraw_f |
// Lraw_g, one slot behind every image launch.
struct DenseFitTap {
  DevBuf packed, info, snaps;
  size_t n_packed, slot, n[5];
  const double* src[5];
  int taken;
  int snap(zigp_ctx* c) {
    double* q = snaps.p + (size_t)taken++ * slot;
    for (int j = 0; j < 5; ++j) {
      if (n[j]) ZIGP_HIP(c, hipMemcpyAsync(q, src[j], sizeof(double) * n[j], hipMemcpyDeviceToDevice, c->stream));
      q += n[j];
    }
    return 0;
  }
};
struct DenseFitNoTap {};
// TAP (zigp_test_dense_fit_update, include/zigp_diag.h): step i's packed vector and Cholesky status come from the caller in place of
// k_gather_rows + dense_step + dense_pack, and the state, the parameter image, the block H and the Lraw blocks are snapshot -- device to
// device, on the loop's stream -- behind every image launch.
template <bool TAP>
int dense_fit_steps(zigp_ctx* c, int32_t mode, bool legacy, const zigp_params* shape, const zigp_fit_opts* o, double* free_state, double* adam_m,
                    double* adam_v, int64_t n_free, int64_t t0, int32_t n_steps, const int64_t* rows, int64_t batch, double jitter, double scale,
                    int32_t include_kl, double* elbo_data, double* kl, const zigp_stage_dense_fit_update* tap = nullptr) {
  if (!c) return ZIGP_EARG;
  const std::string who = legacy ? "zigp_fit_steps" : "zigp_fit_steps_mode";
  auto bad = [&](const char* what) { return fail_arg(c, (who + ": " + what).c_str()); };
  c->dense_fit_steps_applied = 0;      // whatever ends this call early, no update of it has been applied
  if (!shape || !o || !free_state || !adam_m || !adam_v) return bad("NULL argument");
  if (mode != ZIGP_FIT_DIAG && mode != ZIGP_FIT_WHITE && mode != ZIGP_FIT_WHITE_FULL)
    return bad("unknown mode (ZIGP_FIT_DIAG, ZIGP_FIT_WHITE, ZIGP_FIT_WHITE_FULL)");
  const Param par = (Param)mode;
  const bool tri = is_full(par);     // blocks 4, 5 and the packed dLq: the lower triangle of the factor
  if (shape->Mf <= 0 || shape->Mg <= 0 || shape->D <= 0) return bad("need Mf, Mg > 0 and D >= 1");
  if (shape->D > MAXD)
    return bad(("D = " + std::to_string(shape->D) + ": the device fit loop covers D in [1, 8] (zigp_elbo + a host optimiser fit every D up to " ZIGP_MAX_D_STR ")").c_str());
  if (n_steps <= 0 || t0 < 0 || (rows && batch <= 0)) return bad("need n_steps > 0, t0 >= 0 and, with rows, batch > 0");
  if (!(jitter >= 0)) return bad("jitter must be >= 0");
  if (!(o->beta1 >= 0 && o->beta1 < 1 && o->beta2 >= 0 && o->beta2 < 1 && o->eps > 0)) return bad("bad Adam constants");
  const int D = shape->D, M[2] = {shape->Mf, shape->Mg};
  const int es[2] = {o->ell_size_f, o->ell_size_g};
  for (int h = 0; h < 2; ++h)
    if (es[h] != 1 && es[h] != D) return bad("ell_size must be 1 or D");
  if (!c->dX) return bad("no data set (call zigp_set_data first)");
  if (D != c->D) return bad("shape.D differs from the data's D");
  if (legacy && c->q_full) return bad("the full-covariance q(u) is on (zigp_set_q_full, q_diag=False); the device loop fits the diagonal unwhitened parametrisation only (zigp_elbo + a host optimiser)");
  if (legacy && c->whiten) return bad("whitening is on (zigp_set_whiten); the device loop fits the unwhitened parametrisation only (zigp_elbo + a host optimiser)");
  if (c->mean_on) return bad("a mean function is set; its parameters stay with the host loop (zigp_elbo + a host optimiser)");
  {
    std::string kw;
    if (matern_latent(c, kw)) return bad(("a " + kw + " is set (zigp_set_kernel); the device loop fits RBF latents only (zigp_elbo + a host optimiser)").c_str());
  }
  if (c->comm) return bad("a communicator is attached; the dense device loop is single-process");
  if (rows) {
    if ((int64_t)n_steps > ((int64_t)1 << 27) / batch) return bad("n_steps * batch row indices exceed 1 GiB");
    for (int64_t i = 0; i < (int64_t)n_steps * batch; ++i)
      if (rows[i] < 0 || rows[i] >= c->fullN) return bad("row index out of range");
  } else if (c->N <= 0) return bad("no active rows");
  DenseFitArgs fa;
  memset(static_cast<void*>(&fa), 0, sizeof(fa));
  DenseFitDesc& d = fa.d;
  {
    // blocks 4, 5: the diagonal's M entries, or the M (M + 1) / 2 of Lq's lower triangle in row-major order (identity transform)
    const int64_t ns64[2] = {tri ? (int64_t)M[0] * (M[0] + 1) / 2 : M[0], tri ? (int64_t)M[1] * (M[1] + 1) / 2 : M[1]};
    if ((int64_t)(M[0] + M[1]) * (D + 1) + ns64[0] + ns64[1] + 2 * D + 3 > ((int64_t)1 << 30)) return bad("the free state exceeds 2^30 entries");
    const int ns[2] = {(int)ns64[0], (int)ns64[1]};
    const int sizes[DFIT_BLOCKS] = {M[0] * D, M[1] * D, M[0], M[1], ns[0], ns[1], es[0], es[1], 1, 1, 1};
    int off = 0;
    for (int b = 0; b < DFIT_BLOCKS; ++b) {
      d.off[b] = off; d.n[b] = sizes[b]; d.gn[b] = 1; off += sizes[b];
      d.positive[b] = o->positive[b] != 0; d.trainable[b] = o->trainable[b] != 0; d.lr[b] = o->lr[b];
    }
    d.off[DFIT_BLOCKS] = off;
    if ((int64_t)off != n_free) return bad("n_free does not match the model sizes");
    if (tri && (o->positive[4] != 0 || o->positive[5] != 0))
      return bad("positive[4] / positive[5] must be 0 for ZIGP_FIT_WHITE_FULL (the diagonal of a full factor is unconstrained)");
    if (tri)     // a zero diagonal entry: the KL's log is not finite
      for (int h = 0; h < 2; ++h)
        for (int64_t i = 0; i < M[h]; ++i)
          if (free_state[d.off[4 + h] + i * (i + 1) / 2 + i] == 0.0)
            return bad(h ? "the full factor of g has a zero diagonal entry" : "the full factor of f has a zero diagonal entry");
    // the packed result vector (k_dense_pack): header, then per latent dZ (M D), du (M), ds (M; full: dLq's lower triangle), dell (D)
    int g = DP_HDR;
    for (int h = 0; h < 2; ++h) {
      d.goff[0 + h] = g; d.goff[2 + h] = g + M[h] * D; d.goff[4 + h] = g + M[h] * D + M[h]; d.goff[6 + h] = g + M[h] * D + M[h] + ns[h];
      d.gn[6 + h] = es[h] == 1 ? D : 1;
      g += M[h] * D + M[h] + ns[h] + D;
    }
    d.goff[8] = 2; d.goff[9] = 3; d.goff[10] = 4;
  }
  d.tri = tri ? 1 : 0;
  d.D = D; d.M[0] = M[0]; d.M[1] = M[1];
  d.beta1 = o->beta1; d.beta2 = o->beta2; d.eps = o->eps; d.jitter = jitter; d.rtol_eps = c->pivot_rtol * 2.220446049250313e-16;
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(begin_staged_call(c));
  // the call as the step driver sees it: a gradient step over its own gathered batch, or over the active rows
  zigp_params sizes_only;
  memset(&sizes_only, 0, sizeof(sizes_only));
  sizes_only.Mf = M[0]; sizes_only.Mg = M[1]; sizes_only.D = D;
  DenseCall k;
  k.p = &sizes_only; k.D = D; k.jitter = jitter; k.scale = scale; k.g_offset = 0.0; k.include_kl = include_kl; k.predict = false; k.d_out9 = nullptr;
  k.need_grad = true; k.has_rows = true; k.row_begin = 0;
  k.par = par; k.dlq_as_triangle = tri;
  k.hl[0] = HostLatent{M[0], nullptr, nullptr, nullptr, nullptr, 0.0}; k.hl[1] = HostLatent{M[1], nullptr, nullptr, nullptr, nullptr, 0.0};
  k.ell_h[0] = k.ell_h[1] = nullptr;
  const int64_t nidx = rows ? (int64_t)n_steps * batch : 0;
  if (rows) {
    ZIGP_ENSURE(c, c->fitX, (size_t)batch * D); ZIGP_ENSURE(c, c->fitY, (size_t)batch); ZIGP_ENSURE(c, c->fitIdx, (size_t)nidx);
    k.dX = c->fitX.p; k.dY = c->fitY.p; k.Nrows = batch;
  } else { k.dX = c->dX; k.dY = c->dY; k.Nrows = c->N; }
  k.row_end = k.Nrows;
  ZIGP_TRY(dense_plan(c, k));
  // device state of the call: [x | m | v | history (2 per step) | failure record (4 ints) | Cholesky status (2 ints)], all downloaded
  // together at the end, then -- on a 256-byte boundary -- the hyperparameter block
  const size_t nf = (size_t)n_free, n_hist = (size_t)2 * n_steps, n_down = 3 * nf + n_hist + 3, off_hyp = (size_t)round_up((int64_t)n_down, 32);
  ZIGP_ENSURE(c, c->fit, off_hyp + DH_SIZE);
  fa.x = c->fit.p; fa.m = fa.x + nf; fa.v = fa.m + nf; fa.hist = fa.v + nf;
  fa.fail = reinterpret_cast<int*>(fa.hist + n_hist);
  k.d_info2 = fa.fail + 4; fa.info = k.d_info2;
  double* H = c->fit.p + off_hyp;
  k.d_hyp = H;
  size_t off[2][6], total = 0;
  ZIGP_TRY(latents_layout(c, M, D, off, total));
  ZIGP_TRY(latents_views(c, off, D));
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    lt.var = 0.0;            // not read: the kernels take it from the block
    lt.kg_exact = true;      // the per-row form of k_kgrad: the centred form needs a centre chosen from Z and ell, which move on the device
    for (int q = 0; q < WIDE_MAXD; ++q) lt.zc[q] = 0.0;
    if (tri) {     // the M x M buffers of the full factor (latents_upload / latent_qfull_dlq size them for zigp_elbo): before the first step
      const size_t mm = (size_t)M[h] * M[h], mmp = (size_t)lt.Mp * lt.Mp;
      ZIGP_ENSURE(c, lt.Lraw, mm); ZIGP_ENSURE(c, lt.Lq, mmp); ZIGP_ENSURE(c, lt.lqssq, mmp / 256); ZIGP_ENSURE(c, lt.T3, mmp); ZIGP_ENSURE(c, lt.dLq, mmp);
    }
    d.img_Z[h] = (int)off[h][0]; d.img_ell[h] = (int)off[h][1]; d.img_u[h] = (int)off[h][2]; d.img_s[h] = (int)off[h][3]; d.img_Zs[h] = (int)off[h][4];
  }
  const dim3 ugrid(ceil_div(n_free, DFIT_THREADS));
  const dim3 tgrid(ceil_div((int64_t)std::max(M[0], M[1]) * std::max(M[0], M[1]), DFIT_THREADS), 2);
  std::conditional_t<TAP, DenseFitTap, DenseFitNoTap> ts;      // the production loop carries nothing of the hook
  if constexpr (TAP) {
    const size_t n_packed = (size_t)d.goff[7] + D;
    ts.n_packed = n_packed; ts.taken = 0;
    const size_t sn[5] = {3 * nf, total, (size_t)DH_SIZE, tri ? (size_t)M[0] * M[0] : 0, tri ? (size_t)M[1] * M[1] : 0};
    const double* const ssrc[5] = {c->fit.p, c->parm.p, H, c->lat[0].Lraw.p, c->lat[1].Lraw.p};
    ts.slot = 0;
    for (int j = 0; j < 5; ++j) { ts.n[j] = sn[j]; ts.src[j] = ssrc[j]; ts.slot += sn[j]; }
    int64_t f[ZIGP_DFU_COUNT] = {0};
    for (int h = 0; h < 2; ++h) {
      f[ZIGP_DFU_IMG_Z + h] = d.img_Z[h]; f[ZIGP_DFU_IMG_ELL + h] = d.img_ell[h]; f[ZIGP_DFU_IMG_U + h] = d.img_u[h]; f[ZIGP_DFU_IMG_S + h] = d.img_s[h];
      f[ZIGP_DFU_IMG_ZS + h] = d.img_Zs[h]; f[ZIGP_DFU_MP + h] = c->lat[h].Mp;
    }
    f[ZIGP_DFU_N_IMG] = (int64_t)total; f[ZIGP_DFU_N_PACKED] = (int64_t)n_packed; f[ZIGP_DFU_GRID] = ugrid.x; f[ZIGP_DFU_TGRID] = tri ? tgrid.x : 0;
    const int64_t dh[8] = {DH_SIZE, DH_LAT, DH_INV, DH_ELL, DH_SCALE, DH_VAR, DH_PIVTOL, DH_NOISE};
    memcpy(f + ZIGP_DFU_DH_SIZE, dh, sizeof(dh));
    if (tap->facts) memcpy(tap->facts, f, sizeof(f));
    if (!tap->packed) return ZIGP_OK;      // the layout query
    if (!tap->info || tap->n_packed != (int64_t)n_packed || tap->n_img != (int64_t)total) return bad("info missing, or n_packed / n_img differ from the facts");
    ZIGP_ENSURE(c, ts.packed, (size_t)n_steps * n_packed);
    ZIGP_ENSURE(c, ts.info, (size_t)n_steps);      // two ints per step
    ZIGP_ENSURE(c, ts.snaps, (size_t)(1 + n_steps) * ts.slot);
    ZIGP_HIP(c, hipMemcpyAsync(ts.packed.p, tap->packed, sizeof(double) * n_steps * n_packed, hipMemcpyHostToDevice, c->stream));
    ZIGP_HIP(c, hipMemcpyAsync(ts.info.p, tap->info, sizeof(int32_t) * 2 * n_steps, hipMemcpyHostToDevice, c->stream));
  }
  {
    ZIGP_PINNED(c, hst, n_down);
    memcpy(hst, free_state, sizeof(double) * nf); memcpy(hst + nf, adam_m, sizeof(double) * nf); memcpy(hst + 2 * nf, adam_v, sizeof(double) * nf);
    memset(hst + 3 * nf, 0, sizeof(double) * (n_hist + 3));
    ZIGP_HIP(c, hipMemcpyAsync(c->fit.p, hst, sizeof(double) * n_down, hipMemcpyHostToDevice, c->stream));
    ZIGP_HIP(c, hipMemsetAsync(H, 0, sizeof(double) * DH_SIZE, c->stream));
    ZIGP_HIP(c, hipMemsetAsync(c->parm.p, 0, sizeof(double) * total, c->stream));     // the zero padding of Z, u, s, Zs up to Mp
    if (rows) {
      int64_t* hi = (int64_t*)c->pinned.alloc(sizeof(int64_t) * nidx);
      if (!hi) { c->err = "hipHostMalloc failed for the staging arena"; return ZIGP_EHIP; }
      memcpy(hi, rows, sizeof(int64_t) * nidx);
      ZIGP_HIP(c, hipMemcpyAsync(c->fitIdx.p, hi, sizeof(int64_t) * nidx, hipMemcpyHostToDevice, c->stream));
    }
  }
  auto image = [&]() {     // free state -> parameter image, hyperparameter block and, for full factors, the two Lraw blocks
    hipLaunchKernelGGL(k_dense_fit_image, ugrid, dim3(DFIT_THREADS), 0, c->stream, d, fa.x, c->parm.p, H);
    if (tri) hipLaunchKernelGGL(k_dense_fit_image_tri, tgrid, dim3(DFIT_THREADS), 0, c->stream, d, fa.x, c->parm.p, c->lat[0].Lraw.p, c->lat[1].Lraw.p);
  };
  image();
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) ZIGP_TRY(ts.snap(c));
  for (int i = 0; i < n_steps; ++i) {
    if constexpr (TAP) {      // the caller's packed vector and status in place of the step
      ZIGP_HIP(c, hipMemcpyAsync(k.d_info2, ts.info.p + i, sizeof(int) * 2, hipMemcpyDeviceToDevice, c->stream));
      fa.packed = ts.packed.p + (size_t)i * ts.n_packed;
    } else {
      if (rows) {
        hipLaunchKernelGGL(k_gather_rows, dim3(ceil_div(batch * (D + 1), 256)), dim3(256), 0, c->stream, c->fullX, c->fullY,
                           reinterpret_cast<const int64_t*>(c->fitIdx.p) + (int64_t)i * batch, batch, D, c->fitX.p, c->fitY.p);
        ZIGP_HIP(c, hipGetLastError());
      }
      ZIGP_TRY(dense_step(c, k));
      DensePackArgs pa; size_t npk = 0;
      ZIGP_TRY(dense_pack(c, k, pa, npk));
      fa.packed = c->packed.p;
    }
    // lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t counted from 1 (zigp/optim.py AdamGroups.step): the two t-dependent factors from the host
    const double t = (double)(t0 + i + 1);
    fa.step = i; fa.lr_sq = std::sqrt(1.0 - std::pow(d.beta2, t)); fa.lr_den = 1.0 - std::pow(d.beta1, t);
    hipLaunchKernelGGL(k_dense_fit_update, ugrid, dim3(DFIT_THREADS), 0, c->stream, fa);
    image();
    ZIGP_HIP(c, hipGetLastError());
    if constexpr (TAP) ZIGP_TRY(ts.snap(c));
  }
  double* hst = nullptr;
  ZIGP_TRY(download(c, c->fit.p, n_down, &hst));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  const int* hfail = reinterpret_cast<const int*>(hst + 3 * nf + n_hist);
  if constexpr (TAP) {
    if (tap->hist) memcpy(tap->hist, hst + 3 * nf, sizeof(double) * n_hist);
    if (tap->fail) memcpy(tap->fail, hfail, sizeof(int) * 4);
    std::vector<double> hs((size_t)ts.taken * ts.slot);
    ZIGP_HIP(c, hipMemcpy(hs.data(), ts.snaps.p, sizeof(double) * hs.size(), hipMemcpyDeviceToHost));
    double* const dst[7] = {tap->snap_x, tap->snap_m, tap->snap_v, tap->snap_img, tap->snap_H, tap->snap_Lraw[0], tap->snap_Lraw[1]};
    const size_t n[7] = {nf, nf, nf, total, (size_t)DH_SIZE, ts.n[3], ts.n[4]};
    for (int s = 0; s < ts.taken; ++s) {
      const double* q = hs.data() + (size_t)s * ts.slot;
      for (int j = 0; j < 7; ++j) {
        if (dst[j] && n[j]) memcpy(dst[j] + (size_t)s * n[j], q, sizeof(double) * n[j]);
        q += n[j];
      }
    }
  }
  memcpy(free_state, hst, sizeof(double) * nf); memcpy(adam_m, hst + nf, sizeof(double) * nf); memcpy(adam_v, hst + 2 * nf, sizeof(double) * nf);
  const int done = hfail[0] ? hfail[0] - 1 : n_steps;       // steps whose update was applied
  c->dense_fit_steps_applied = done;
  for (int i = 0; i < n_steps; ++i) {
    if (elbo_data) elbo_data[i] = i < done ? hst[3 * nf + 2 * i] : NAN;
    if (kl) kl[i] = i < done ? hst[3 * nf + 2 * i + 1] : NAN;
  }
  if (hfail[0]) {
    char b[320];
    snprintf(b, sizeof(b), "Cholesky failed in step %d of this %s call (iteration %lld): Kuu of latent %s not positive definite at pivot %d; "
             "the state returned is the one before that step", hfail[0] - 1, who.c_str(), (long long)(t0 + hfail[0] - 1), hfail[1] ? "g" : "f", hfail[2]);
    c->err = b; c->info = hfail[2];
    return ZIGP_ENOTPD;
  }
  return ZIGP_OK;
}
}  // namespace
extern "C" {
int zigp_fit_steps(zigp_ctx* c, const zigp_params* shape, const zigp_fit_opts* o, double* free_state, double* adam_m, double* adam_v, int64_t n_free,
                   int64_t t0, int32_t n_steps, const int64_t* rows, int64_t batch, double jitter, double scale, int32_t include_kl, double* elbo_data,
                   double* kl) {
  return dense_fit_steps<false>(c, ZIGP_FIT_DIAG, true, shape, o, free_state, adam_m, adam_v, n_free, t0, n_steps, rows, batch, jitter, scale, include_kl,
                                elbo_data, kl);
}
int zigp_fit_steps_mode(zigp_ctx* c, int32_t mode, const zigp_params* shape, const zigp_fit_opts* o, double* free_state, double* adam_m,
                        double* adam_v, int64_t n_free, int64_t t0, int32_t n_steps, const int64_t* rows, int64_t batch, double jitter,
                        double scale, int32_t include_kl, double* elbo_data, double* kl) {
  return dense_fit_steps<false>(c, mode, false, shape, o, free_state, adam_m, adam_v, n_free, t0, n_steps, rows, batch, jitter, scale, include_kl,
                                elbo_data, kl);
}
int64_t zigp_fit_steps_applied(zigp_ctx* c) { return c ? c->dense_fit_steps_applied : (int64_t)ZIGP_EARG; }

// The image and update kernels of the dense fit loop through dense_fit_steps itself (include/zigp_diag.h): full-batch steps over the
// active rows, none of which runs.
int zigp_test_dense_fit_update(zigp_ctx* c, const zigp_stage_dense_fit_update* s) {
  if (!c) return ZIGP_EARG;
  if (!s || s->n_steps > 4096) return fail_arg(c, "zigp_test_dense_fit_update: bad arguments");
  const int rc = dense_fit_steps<true>(c, s->mode, false, s->shape, s->opts, s->x, s->m, s->v, s->n_free, s->t0, s->n_steps, nullptr, 0, s->jitter, 1.0, 1,
                                       s->elbo_data, s->kl, s);
  if (s->steps_applied) *s->steps_applied = c->dense_fit_steps_applied;
  return rc;
}

int zigp_predict(zigp_ctx* c, const zigp_params* p, const double* Xnew, int64_t N, double jitter, double g_offset, double* out9) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  if (N < 0 || (N > 0 && (!Xnew || !out9))) return fail_arg(c, "zigp_predict: bad arguments");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  PredRows r;   // the block itself is the result: nine rows from its first, m0
  ZIGP_TRY(rows_from_predict(c, p, Xnew, nullptr, N, jitter, g_offset, false, r));
  return finish_copies(c, {{out9, r.m0, (size_t)9 * N}});
}

int zigp_predict_device(zigp_ctx* c, const zigp_params* p, const double* dXnew, int64_t N, double jitter, double g_offset, double* d_out9) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  if (N < 0 || (N > 0 && (!dXnew || !d_out9))) return fail_arg(c, "zigp_predict_device: bad arguments");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(require_device_ptrs(c, {dXnew, d_out9}, "zigp_predict_device: Xnew and out9 must be device memory of the context's GPU"));
  // rows in place: no copy in, no copy out; the call is complete on return (run_dense ends with the stream's synchronisation)
  return run_dense(c, p, dXnew, nullptr, N, p->D, jitter, 1.0, g_offset, 0, N, 0, true, d_out9, nullptr, nullptr, nullptr);
}

// ---- the heads on the dense path (include/zigp.h): latent f under a Gaussian or a Bernoulli likelihood ----
}  // extern "C"
namespace {
// The refusals every head entry shares, then `q`: the caller's f half with the placeholder latent in the g fields.  validate_params' rules
// for latent f alone: the g fields of `p` and the kernel of latent g (zigp_set_kernel(ctx, 1, ...)) are not read.
int head_params(zigp_ctx* c, const char* who, const zigp_params* p, int32_t lik, zigp_params& q) {
  const std::string w(who);
  if (lik != ZIGP_LIK_GAUSSIAN && lik != ZIGP_LIK_BERNOULLI) return refuse(c, w, "lik must be ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI");
  if (c->comm) return refuse(c, w, "a communicator is attached (zigp_comm_init); the heads on the dense path are single-process");
  if (!p) return refuse(c, w, "params is NULL");
  if (p->Mf <= 0) return refuse(c, w, "params.Mf must be positive");
  if (p->D <= 0 || p->D > ZIGP_MAX_D) return refuse(c, w, "params.D must be in [1, " ZIGP_MAX_D_STR "] (ZIGP_MAX_D)");
  if (p->D > MAXD && is_matern(c->kern[0]))
    return refuse(c, w, std::string("a ") + kern_name(c->kern[0]) + " kernel on latent f (zigp_set_kernel) and params.D = " + std::to_string(p->D) +
                            ": the Matern kernels cover D in [1, 8] (the wide kernels are RBF only)");
  if (p->D > MAXD && c->mean_on)
    for (int d = 0; d < MAXD; ++d)
      if (c->mean_a[d] != 0.0) return refuse(c, w, "a Linear mean function is set and params.D > 8: Linear covers D in [1, 8] (Zero and Constant work at every D)");
  if (!p->Zf || !p->u_fm || !p->u_fs_sqrt || !p->ell_f) return refuse(c, w, "NULL pointer in params (Zf, u_fm, u_fs_sqrt, ell_f)");
  if (!(p->var_f > 0)) return refuse(c, w, "params.var_f must be positive");
  if (lik == ZIGP_LIK_GAUSSIAN && !(p->noise > 0)) return refuse(c, w, "params.noise must be positive (ZIGP_LIK_GAUSSIAN)");
  for (int d = 0; d < p->D; ++d)
    if (!(p->ell_f[d] > 0)) return refuse(c, w, "params.ell_f: lengthscales must be positive");
  if (c->q_full) {
    if (!c->whiten) return refuse(c, w, "zigp_set_q_full is on while whitening is off: the full-covariance q(u) exists for the whitened model only (zigp_set_whiten)");
    for (int m = 0; m < p->Mf; ++m)
      if (!(p->u_fs_sqrt[(size_t)m * p->Mf + m] != 0)) return refuse(c, w, "params.u_fs_sqrt has a zero (or NaN) diagonal entry (full q_sqrt, zigp_set_q_full)");
  } else {
    for (int m = 0; m < p->Mf; ++m)
      if (!(p->u_fs_sqrt[m] > 0)) return refuse(c, w, "params.u_fs_sqrt must be positive (diagonal q_sqrt, transforms.positive)");
  }
  const HeadPlaceholder& h = head_placeholder();
  q = *p;
  q.Mg = 1; q.Zg = h.Z; q.u_gm = h.u; q.u_gs_sqrt = h.s; q.ell_g = h.ell; q.var_g = 1.0;
  if (lik == ZIGP_LIK_BERNOULLI) q.noise = 1.0;     // not read by the Bernoulli head; its gradient comes back 0
  return 0;
}
}  // namespace
extern "C" {

int zigp_head_elbo(zigp_ctx* c, const zigp_params* p, int32_t lik, double jitter, double scale, int64_t row_begin, int64_t row_end,
                   int32_t include_kl, double* elbo_data, double* kl, zigp_grads* grads) {
  if (!c) return ZIGP_EARG;
  zigp_params q;
  ZIGP_TRY(head_params(c, "zigp_head_elbo", p, lik, q));
  if (!c->dX) return fail_arg(c, "zigp_head_elbo: no data set (call zigp_set_data first)");
  if (p->D != c->D) return fail_arg(c, "zigp_head_elbo: params.D differs from the data's D");
  if (row_begin < 0 || row_end > c->N || row_begin > row_end) return fail_arg(c, "zigp_head_elbo: bad row range");
  if (!(jitter >= 0)) return fail_arg(c, "zigp_head_elbo: jitter must be >= 0");
  ZIGP_HIP(c, hipSetDevice(c->device));
  return run_dense_lik(c, &q, lik, c->dX, c->dY, c->N, c->D, jitter, scale, 0.0, row_begin, row_end, include_kl, false, nullptr, elbo_data, kl,
                       grads);
}

int zigp_head_predict(zigp_ctx* c, const zigp_params* p, int32_t lik, const double* Xnew, int64_t N, double jitter, double* out4) {
  if (!c) return ZIGP_EARG;
  zigp_params q;
  ZIGP_TRY(head_params(c, "zigp_head_predict", p, lik, q));
  if (N < 0 || (N > 0 && (!Xnew || !out4))) return fail_arg(c, "zigp_head_predict: bad arguments (Xnew, N, out4)");
  if (!(jitter >= 0)) return fail_arg(c, "zigp_head_predict: jitter must be >= 0");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  const double* dX = nullptr;
  ZIGP_TRY(stage_inputs(c, Xnew, N, q.D, false, &dX));
  ZIGP_ENSURE(c, c->out9, (size_t)9 * N);     // the predict block of the row calls; a head fills its first four rows
  ZIGP_TRY(run_dense_lik(c, &q, lik, dX, nullptr, N, q.D, jitter, 1.0, 0.0, 0, N, 0, true, c->out9.p, nullptr, nullptr, nullptr));
  return finish_copies(c, {{out4, c->out9.p, (size_t)4 * N}});
}

int zigp_head_predict_device(zigp_ctx* c, const zigp_params* p, int32_t lik, const double* dXnew, int64_t N, double jitter, double* d_out4) {
  if (!c) return ZIGP_EARG;
  zigp_params q;
  ZIGP_TRY(head_params(c, "zigp_head_predict_device", p, lik, q));
  if (N < 0 || (N > 0 && (!dXnew || !d_out4))) return fail_arg(c, "zigp_head_predict_device: bad arguments (Xnew, N, out4)");
  if (!(jitter >= 0)) return fail_arg(c, "zigp_head_predict_device: jitter must be >= 0");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(require_device_ptrs(c, {dXnew, d_out4}, "zigp_head_predict_device: Xnew and out4 must be device memory of the context's GPU"));
  return run_dense_lik(c, &q, lik, dXnew, nullptr, N, q.D, jitter, 1.0, 0.0, 0, N, 0, true, d_out4, nullptr, nullptr, nullptr);
}

int zigp_prior_kl(zigp_ctx* c, const zigp_params* p, double jitter, double* kl2) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  if (!kl2) return fail_arg(c, "zigp_prior_kl: kl2 is NULL");
  ZIGP_HIP(c, hipSetDevice(c->device));
  HostLatent hl[2] = {{p->Mf, p->Zf, p->u_fm, p->u_fs_sqrt, p->ell_f, p->var_f, c->kern[0]},
                      {p->Mg, p->Zg, p->u_gm, p->u_gs_sqrt, p->ell_g, p->var_g, c->kern[1]}};
  ZIGP_TRY(begin_staged_call(c));
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  const Param par = param_of(c);
  ZIGP_TRY(latents_upload(c, hl, p->D, par));
  ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
  ZIGP_TRY(latents_forward(c, hl, p->D, jitter, par, true, false, nullptr, nullptr));
  ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  double klh[2] = {0.0, 0.0};
  for (int h = 0; h < 2; ++h)
    ZIGP_HIP(c, hipMemcpyAsync(&klh[h], (is_white(par) ? c->lat[h].wh.p : c->lat[h].vec.p) + 3 * c->lat[h].Mp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ZIGP_TRY(check_info(c, "Kuu"));          // synchronises; on failure kl2 is left untouched
  kl2[0] = klh[0]; kl2[1] = klh[1];
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  return ZIGP_OK;
}

int zigp_rbf_K(zigp_ctx* c, const double* X1, int64_t n1, const double* X2, int64_t n2, int32_t D, const double* ell, double var, double* K) {
  if (!c) return ZIGP_EARG;
  if (!X1 || n1 <= 0 || D <= 0 || !ell || !K) return fail_arg(c, "zigp_rbf_K: bad arguments");
  if (D > ZIGP_MAX_D) return fail_arg(c, "zigp_rbf_K: D must be in [1, " ZIGP_MAX_D_STR "] (ZIGP_MAX_D)");
  if (!X2) n2 = n1;
  if (n2 <= 0) return fail_arg(c, "zigp_rbf_K: bad n2");
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_ENSURE(c, c->scratch, (size_t)(n1 + n2) * D);
  ZIGP_ENSURE(c, c->scratch2, (size_t)n1 * n2);
  double* d1 = c->scratch.p; double* d2 = d1 + n1 * D;
  ZIGP_HIP(c, hipMemcpyAsync(d1, X1, sizeof(double) * n1 * D, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(d2, X2 ? X2 : X1, sizeof(double) * n2 * D, hipMemcpyHostToDevice, c->stream));
  if (D > MAXD)
    hipLaunchKernelGGL(k_rbf_matrix_wide, dim3(ceil_div(n1 * n2, 256)), dim3(256), 0, c->stream, d1, n1, d2, n2, make_hyp_wide(ell, var, D), 0.0,
                       c->scratch2.p, n1, n2, n2);
  else {
    KernHyp h = make_hyp(ell, var, D);
    hipLaunchKernelGGL(k_rbf_matrix, dim3(ceil_div(n1 * n2, 256)), dim3(256), 0, c->stream, d1, n1, d2, n2, h, 0.0, c->scratch2.p, n1, n2, n2);
  }
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_HIP(c, hipMemcpyAsync(K, c->scratch2.p, sizeof(double) * n1 * n2, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_kern_K(zigp_ctx* c, int32_t kind, const double* X1, int64_t n1, const double* X2, int64_t n2, int32_t D, const double* ell, double var,
                double* K) {
  if (!c) return ZIGP_EARG;
  if (kind == ZIGP_KERN_RBF) return zigp_rbf_K(c, X1, n1, X2, n2, D, ell, var, K);
  if (kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52)
    return fail_arg(c, "zigp_kern_K: unknown kernel kind (ZIGP_KERN_RBF, ZIGP_KERN_MATERN32, ZIGP_KERN_MATERN52)");
  if (!X1 || n1 <= 0 || D <= 0 || !ell || !K) return fail_arg(c, "zigp_kern_K: bad arguments");
  if (D > MAXD) return fail_arg(c, (std::string("zigp_kern_K: the ") + kern_name(kind) + " kernel covers D in [1, 8]").c_str());
  if (!X2) n2 = n1;
  if (n2 <= 0) return fail_arg(c, "zigp_kern_K: bad n2");
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_ENSURE(c, c->scratch, (size_t)(n1 + n2) * D);
  ZIGP_ENSURE(c, c->scratch2, (size_t)n1 * n2);
  double* d1 = c->scratch.p; double* d2 = d1 + n1 * D;
  ZIGP_HIP(c, hipMemcpyAsync(d1, X1, sizeof(double) * n1 * D, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(d2, X2 ? X2 : X1, sizeof(double) * n2 * D, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_matern_matrix, dim3(ceil_div(n1 * n2, 256)), dim3(256), 0, c->stream, d1, n1, d2, n2, make_hyp(ell, var, D), kind, c->scratch2.p);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_HIP(c, hipMemcpyAsync(K, c->scratch2.p, sizeof(double) * n1 * n2, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_profile_enable(zigp_ctx* c, int32_t on) { if (!c) return ZIGP_EARG; c->prof_on = on != 0; return ZIGP_OK; }
int zigp_profile_reset(zigp_ctx* c) {
  if (!c) return ZIGP_EARG;
  prof_collect(c);
  for (int i = 0; i < ZIGP_NCLASS; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; c->prof_flops[i] = 0; c->prof_total[i] = 0; }
  return ZIGP_OK;
}
int zigp_profile_get(zigp_ctx* c, double* ms, int64_t* launches, double* flops) {
  if (!c) return ZIGP_EARG;
  prof_collect(c);
  for (int i = 0; i < ZIGP_NCLASS; ++i) { if (ms) ms[i] = c->prof_ms[i]; if (launches) launches[i] = c->prof_n[i]; if (flops) flops[i] = c->prof_flops[i]; }
  return ZIGP_OK;
}
int zigp_profile_sampling(zigp_ctx* c, int32_t every) {
  if (!c) return ZIGP_EARG;
  if (every < 1) return fail_arg(c, "zigp_profile_sampling: every must be >= 1");
  c->prof_every = every;
  return ZIGP_OK;
}
int zigp_profile_totals(zigp_ctx* c, int64_t* total_launches) {
  if (!c || !total_launches) return ZIGP_EARG;
  for (int i = 0; i < ZIGP_NCLASS; ++i) total_launches[i] = c->prof_total[i];
  return ZIGP_OK;
}

// ---- sustained shader clock (bench.py) ------------------------------------------------------------
// One workgroup per XCD (workgroups of a dispatch go round-robin over the 8 XCDs): lane 0 records its XCC id, the shader-clock counter
// (s_memtime) and the constant 100 MHz counter (s_memrealtime).  Two calls bracket a measured region; the host pairs the stamps by XCC id.
__global__ void k_clock_stamp(long long* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const unsigned xcc = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) & 0xf;     // HW_REG_XCC_ID, bits [3:0]
  const long long cyc = (long long)__builtin_readcyclecounter();
  const long long rt = (long long)__builtin_amdgcn_s_memrealtime();
  out[3 * blockIdx.x + 0] = (long long)xcc;
  out[3 * blockIdx.x + 1] = cyc;
  out[3 * blockIdx.x + 2] = rt;
}
int zigp_clock_stamp(zigp_ctx* c, int64_t* out) {
  if (!c || !out) return ZIGP_EARG;
  static_assert(sizeof(long long) == sizeof(int64_t), "stamp layout");
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_ENSURE(c, c->scratch2, 64);
  hipLaunchKernelGGL(k_clock_stamp, dim3(8), dim3(64), 0, c->stream_main, reinterpret_cast<long long*>(c->scratch2.p));
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_HIP(c, hipMemcpyAsync(out, c->scratch2.p, sizeof(int64_t) * 24, hipMemcpyDeviceToHost, c->stream_main));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream_main));
  return ZIGP_OK;
}

// ---- diagnostics -------------------------------------------------------------------------------
int zigp_test_kuf(zigp_ctx* c, int64_t N, int32_t M, int32_t D, const double* X, const double* Z, const double* ell, double var, double* K) {
  if (!c) return ZIGP_EARG;
  if (N <= 0 || M <= 0 || D < 1 || D > ZIGP_MAX_D || !X || !Z || !ell || !K) return fail_arg(c, "zigp_test_kuf: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int64_t Nc = round_up(N, 1024);
  const int Mp = (int)round_up(M, 16);
  const KufHypWide khw = make_kuf_hyp_wide(ell, var, D);
  KufHyp kh;
  for (int d = 0; d < MAXD; ++d) kh.scale[d] = khw.scale[d];
  kh.var = var;
  std::vector<double> zs((size_t)Mp * D, 0.0), hk((size_t)Mp * Nc);
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < D; ++d) zs[(size_t)m * D + d] = Z[(size_t)m * D + d] * khw.scale[d];
  DevBuf dx, dz, dk;
  ZIGP_ENSURE(c, dx, (size_t)N * D); ZIGP_ENSURE(c, dz, zs.size()); ZIGP_ENSURE(c, dk, hk.size());
  ZIGP_HIP(c, hipMemcpyAsync(dx.p, X, sizeof(double) * N * D, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(dz.p, zs.data(), sizeof(double) * zs.size(), hipMemcpyHostToDevice, c->stream));
  const dim3 grid((unsigned)(Nc / 512), Mp / 16), block(256);
#define ZIGP_KUF(DD) \
  case DD: hipLaunchKernelGGL((k_kuf_build<DD, KufHyp>), grid, block, 0, c->stream, dx.p, N, (int64_t)0, dz.p, M, kh, dk.p, Nc); break;
  switch (D) {
    ZIGP_KUF(1) ZIGP_KUF(2) ZIGP_KUF(3) ZIGP_KUF(4) ZIGP_KUF(5) ZIGP_KUF(6) ZIGP_KUF(7) ZIGP_KUF(8)
    default: hipLaunchKernelGGL(k_kuf_build_wide, grid, block, 0, c->stream, dx.p, N, (int64_t)0, dz.p, M, D, khw, dk.p, Nc); break;
  }
#undef ZIGP_KUF
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_HIP(c, hipMemcpyAsync(hk.data(), dk.p, sizeof(double) * hk.size(), hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  for (int m = 0; m < M; ++m) memcpy(K + (size_t)m * N, &hk[(size_t)m * Nc], sizeof(double) * N);
  return ZIGP_OK;
}

int zigp_test_kuf_kind(zigp_ctx* c, int32_t kind, int64_t N, int32_t M, int32_t D, const double* X, const double* Z, const double* ell, double var,
                       double* K, double* Kd) {
  if (!c) return ZIGP_EARG;
  if (kind != ZIGP_KERN_RBF && kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52) return fail_arg(c, "zigp_test_kuf_kind: unknown kernel kind");
  if (N <= 0 || M <= 0 || D < 1 || D > ZIGP_MAX_D || !X || !Z || !ell || !K) return fail_arg(c, "zigp_test_kuf_kind: bad arguments");
  if (is_matern(kind) && D > MAXD) return fail_arg(c, (std::string("zigp_test_kuf_kind: the ") + kern_name(kind) + " kernel covers D in [1, 8]").c_str());
  ZIGP_HIP(c, hipSetDevice(c->device));
  // the panel through the chunk loop's own launch helper, on a latent of this call's own
  const int64_t Nc = round_up(N, 1024);
  Latent lt;
  lt.M = M; lt.Mp = (int)round_up(M, BM); lt.var = var;
  const int Mp = lt.Mp, Mp16 = (int)round_up(M, 16);
  const KufHypWide khw = make_kuf_hyp_wide(ell, var, D);
  std::vector<double> zs((size_t)Mp * D, 0.0), hk((size_t)Mp16 * Nc);
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < D; ++d) zs[(size_t)m * D + d] = Z[(size_t)m * D + d] * khw.scale[d];
  DevBuf dx;
  ZIGP_ENSURE(c, dx, (size_t)N * D); ZIGP_ENSURE(c, lt.Zs, zs.size()); ZIGP_ENSURE(c, lt.K, (size_t)Mp * Nc);
  if (Kd && is_matern(kind)) ZIGP_ENSURE(c, lt.Kd, (size_t)Mp * Nc);
  ZIGP_HIP(c, hipMemcpyAsync(dx.p, X, sizeof(double) * N * D, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(lt.Zs.p, zs.data(), sizeof(double) * zs.size(), hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemsetAsync(lt.K.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * (size_t)Mp * Nc, c->stream));
  if (lt.Kd.p) ZIGP_HIP(c, hipMemsetAsync(lt.Kd.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * (size_t)Mp * Nc, c->stream));
  ZIGP_TRY(latent_chunk_kuf(c, lt, dx.p, N, 0, Nc, D, ell, nullptr, kind, Kd != nullptr));
  for (int pass = 0; pass < 2; ++pass) {
    double* dst = pass ? Kd : K;
    if (!dst) continue;
    const double* src = (pass && is_matern(kind)) ? lt.Kd.p : lt.K.p;      // RBF: K' = K
    ZIGP_HIP(c, hipMemcpyAsync(hk.data(), src, sizeof(double) * hk.size(), hipMemcpyDeviceToHost, c->stream));
    ZIGP_HIP(c, hipStreamSynchronize(c->stream));
    for (int m = 0; m < Mp16; ++m) memcpy(dst + (size_t)m * N, &hk[(size_t)m * Nc], sizeof(double) * N);
  }
  return ZIGP_OK;
}

int zigp_test_kgmom_list(int32_t M, int64_t Nc, int64_t cap, int64_t* out) {
  // host only: the list run_dense plans for the moments product of the wide Kuf gradient -- out[0] = slices, out[1] = entries per
  // workgroup, out[2] = entries, then (bi, bj, kbeg, kend, slice) per entry, as many as fit `cap` int64
  if (M <= 0 || Nc <= 0 || Nc % 1024 != 0 || !out || cap < 3) return ZIGP_EARG;
  const int nbm = (int)(round_up(M, BM) / BM);
  std::vector<GemmTile> v;
  out[0] = kgmom_slices(nbm, Nc); out[1] = kgmom_tiles(nbm, Nc).build(v); out[2] = (int64_t)v.size();
  for (size_t i = 0; i < v.size() && 3 + 5 * (int64_t)(i + 1) <= cap; ++i) {
    int64_t* o = out + 3 + 5 * i;
    o[0] = v[i].bi; o[1] = v[i].bj; o[2] = v[i].kbeg; o[3] = v[i].kend; o[4] = v[i].slice;
  }
  return ZIGP_OK;
}

int zigp_test_sk_list(int32_t rule, int32_t nb, int64_t cap, int64_t* out) {
  // host only: the split-K list of a k-range rule (zigp_host.h SkRule) at nb blocks, through run_gemm_sk's own builder -- out[0] = slices,
  // out[1] = lower_only of the finish pass, out[2] = entries, then (bi, bj, kbeg, kend, slice) per entry, as many as fit `cap` int64
  if (rule < 0 || rule >= (int)SkRule::COUNT || nb <= 0 || !out || cap < 3) return ZIGP_EARG;
  std::vector<GemmTile> v;
  build_sk_list((SkRule)rule, nb, v);
  out[0] = sk_slices((SkRule)rule, nb); out[1] = SK_RULES[rule].lower_only ? 1 : 0; out[2] = (int64_t)v.size();
  for (size_t i = 0; i < v.size() && 3 + 5 * (int64_t)(i + 1) <= cap; ++i) {
    int64_t* o = out + 3 + 5 * i;
    o[0] = v[i].bi; o[1] = v[i].bj; o[2] = v[i].kbeg; o[3] = v[i].kend; o[4] = v[i].slice;
  }
  return ZIGP_OK;
}

int zigp_test_trmm_list(int32_t lower, int32_t Mf, int32_t Mg, int64_t Nc, int32_t tail_on, int64_t* out) {
  // host only (no context, no GPU): the lists run_dense plans for A1 (lower) or A2 (upper) of a chunk of Nc rows, checked tile by tile
  if (Mf <= 0 || Mg <= 0 || Nc <= 0 || Nc % BN != 0 || !out) return ZIGP_EARG;
  const int Mp[2] = {(int)round_up(Mf, BM), (int)round_up(Mg, BM)}, nbn = (int)(Nc / BN), kb = BM / BK;
  const ChunkPlan pl = chunk_plan({Mf, Mg}, Nc, Param::Diag, false, tail_on != 0, false);
  int64_t wgs[2], per[2], worst_tail = 0;
  for (int h = 0; h < 2; ++h) {
    const int nbm = Mp[h] / BM;
    std::vector<GemmTile> v;
    per[h] = (lower ? pl.lat[h].a1_spec : pl.lat[h].a2j_spec).build(v);
    if (v.size() % (size_t)per[h]) return -10;
    wgs[h] = (int64_t)(v.size() / per[h]);
    std::vector<int> seen((size_t)nbm * nbn, 0);
    for (const GemmTile& t : v) {
      if (t.kend <= t.kbeg) continue;                                   // padding
      if (t.bi < 0 || t.bi >= nbm || t.bj < 0 || t.bj >= nbn) return -11;
      const int k0 = lower ? 0 : t.bi * kb, k1 = lower ? (t.bi + 1) * kb : nbm * kb;
      if (t.kbeg != k0 || t.kend != k1 || (t.kdir != 1 && t.kdir != -1) || t.slice != 0) return -12;   // the whole k range of its row block, nothing else
      seen[(size_t)t.bi * nbn + t.bj] += 1;
    }
    for (int q : seen) if (q != 1) return -13;                          // every tile exactly once
    if (pl.paired && pl.tail.units[h] > 0) {                            // workgroups behind the regular units: the LPT tail
      const int64_t regular = wgs[h] - 8 * (int64_t)std::min(64, pl.tail.bins[h]);
      for (int64_t w = std::max<int64_t>(regular, 0); w < wgs[h]; ++w) {
        int64_t load = 0;
        for (int e = 0; e < per[h]; ++e) { const GemmTile& t = v[(size_t)w * per[h] + e]; load += std::max(0, t.kend - t.kbeg) / kb; }
        worst_tail = std::max(worst_tail, load);
      }
    }
  }
  out[0] = wgs[0]; out[1] = wgs[1]; out[2] = per[0]; out[3] = per[1]; out[4] = pl.tail.units[0]; out[5] = pl.tail.units[1]; out[6] = worst_tail; out[7] = pl.paired ? 1 : 0;
  return ZIGP_OK;
}

int zigp_test_gemm(zigp_ctx* c, int32_t transA, int32_t transB, int64_t m, int64_t n, int64_t k, const double* A, const double* B, double* C) {
  if (!c) return ZIGP_EARG;
  if (m <= 0 || n <= 0 || k <= 0 || !A || !B || !C) return fail_arg(c, "zigp_test_gemm: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int64_t mp = round_up(m, BM), np = round_up(n, BN), kp = round_up(k, BM);
  // stored shapes: A is (m,k) or (k,m) if transA; B is (k,n) or (n,k) if transB
  const int64_t ar = transA ? kp : mp, ac = transA ? mp : kp, br = transB ? np : kp, bc = transB ? kp : np;
  std::vector<double> ha((size_t)ar * ac, 0.0), hb((size_t)br * bc, 0.0), hc((size_t)mp * np);
  const int64_t ar0 = transA ? k : m, ac0 = transA ? m : k, br0 = transB ? n : k, bc0 = transB ? k : n;
  for (int64_t i = 0; i < ar0; ++i) memcpy(&ha[i * ac], &A[i * ac0], sizeof(double) * ac0);
  for (int64_t i = 0; i < br0; ++i) memcpy(&hb[i * bc], &B[i * bc0], sizeof(double) * bc0);
  DevBuf da, db, dc;
  ZIGP_ENSURE(c, da, ha.size()); ZIGP_ENSURE(c, db, hb.size()); ZIGP_ENSURE(c, dc, hc.size());
  ZIGP_HIP(c, hipMemcpyAsync(da.p, ha.data(), sizeof(double) * ha.size(), hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(db.p, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, c->stream));
  TileList tl;
  ZIGP_TRY(tiles_full(c, (int)(mp / BM), (int)(np / BN), (int)(kp / BK), tl));
  GemmArgs g = mk_args(da.p, ac, db.p, bc, dc.p, np);
  if (!transA && !transB) ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_MNCONTIG, false>(c, tl, g, EpiStore())));
  if (transA && !transB) ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false>(c, tl, g, EpiStore())));
  if (!transA && transB) ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_KCONTIG, false>(c, tl, g, EpiStore())));
  if (transA && transB) ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_KCONTIG, false>(c, tl, g, EpiStore())));
  ZIGP_HIP(c, hipMemcpyAsync(hc.data(), dc.p, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < m; ++i) memcpy(&C[i * n], &hc[i * np], sizeof(double) * n);
  return ZIGP_OK;
}

int zigp_test_potrf_trtri(zigp_ctx* c, int64_t n, const double* A, double* L, double* W, int32_t split_k) {
  if (!c) return ZIGP_EARG;
  if (n <= 0 || !A) return fail_arg(c, "zigp_test_potrf_trtri: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int Mp = (int)round_up(n, BM);
  std::vector<double> ha((size_t)Mp * Mp, 0.0);
  for (int64_t i = 0; i < Mp; ++i) {
    if (i < n) memcpy(&ha[i * Mp], &A[i * n], sizeof(double) * n);
    else ha[i * Mp + i] = 1.0;
  }
  DevBuf dl, dw, dt, dplanes;
  ZIGP_ENSURE(c, dl, ha.size()); ZIGP_ENSURE(c, dw, ha.size()); ZIGP_ENSURE(c, dt, ha.size());
  ZIGP_HIP(c, hipMemcpyAsync(dl.p, ha.data(), sizeof(double) * ha.size(), hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  if (split_k) {     // the chain as the dense M x M forward runs it: every block product cut into k slices (run_gemm_sk_tiles)
    const PotrfJob job = {dl.p, dw.p, dt.p, Mp, true, (int)n, 0.0, false, &dplanes};
    const hipStream_t st = c->stream;
    ZIGP_TRY(potrf_trtri_jobs(c, 1, &job, &st));
  } else ZIGP_TRY(potrf_trtri(c, dl.p, dw.p, dt.p, Mp, true, (int)n));
  ZIGP_TRY(check_info(c, "A"));
  std::vector<double> ho(ha.size());
  if (L) {
    ZIGP_HIP(c, hipMemcpyAsync(ho.data(), dl.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, c->stream));
    ZIGP_HIP(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; ++i) memcpy(&L[i * n], &ho[i * Mp], sizeof(double) * n);
  }
  if (W) {
    ZIGP_HIP(c, hipMemcpyAsync(ho.data(), dw.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, c->stream));
    ZIGP_HIP(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; ++i) memcpy(&W[i * n], &ho[i * Mp], sizeof(double) * n);
  }
  return 0;
}

static_assert(PT_REC == ZIGP_PSF_PER && PT_DIAG == ZIGP_PSL_DIAG && PT_TRI2 == ZIGP_PSL_TRI2, "the tap's records are the hook's facts");
int zigp_test_potrf_stages(zigp_ctx* c, const zigp_stage_potrf* a) {
  if (!c) return ZIGP_EARG;
  if (!a || a->n < 1 || a->n > 4096 || !a->A) return fail_arg(c, "zigp_test_potrf_stages: bad arguments");
  const int n = (int)a->n, Mp = (int)round_up(n, BM), nb = Mp / BM;
  int levels = 0;
  for (int b = 1; b < nb; b *= 2) ++levels;
  const int launches = nb + 2 * (nb - 1) + 2 * levels, images = launches + nb;
  if (a->facts && a->facts_cap < ZIGP_PSF_REC + (int64_t)PT_REC * launches) return fail_arg(c, "zigp_test_potrf_stages: facts_cap too small");
  if (a->snap && a->snap_cap < images) return fail_arg(c, "zigp_test_potrf_stages: snap_cap too small");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const size_t mm = (size_t)Mp * Mp;
  std::vector<double> ha(mm, 0.0);
  for (int64_t i = 0; i < Mp; ++i) {
    if (i < n) memcpy(&ha[i * Mp], &a->A[i * n], sizeof(double) * n);
    else ha[i * Mp + i] = 1.0;
  }
  DevBuf dl, dw, dt, dplanes, dsnap;
  ZIGP_ENSURE(c, dl, mm); ZIGP_ENSURE(c, dw, mm); ZIGP_ENSURE(c, dt, mm);
  if (a->snap) ZIGP_ENSURE(c, dsnap, mm * images);
  ZIGP_HIP(c, hipMemcpyAsync(dl.p, ha.data(), sizeof(double) * mm, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemsetAsync(dt.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * mm, c->stream));   // T "as left": what no launch wrote holds the sentinel
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  PotrfTap tap;
  tap.snap = a->snap ? dsnap.p : nullptr;
  tap.cap = images;
  const PotrfJob job = {dl.p, dw.p, dt.p, Mp, true, n, 0.0, false, a->split_k ? &dplanes : nullptr};
  const hipStream_t st = c->stream;
  ZIGP_TRY(potrf_trtri_jobs(c, 1, &job, &st, &tap));
  int h = 0;
  ZIGP_HIP(c, hipMemcpyAsync(&h, c->d_info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));     // the one synchronisation; everything below is a download
  if (a->L) ZIGP_HIP(c, hipMemcpy(a->L, dl.p, sizeof(double) * mm, hipMemcpyDeviceToHost));
  if (a->W) ZIGP_HIP(c, hipMemcpy(a->W, dw.p, sizeof(double) * mm, hipMemcpyDeviceToHost));
  if (a->T) ZIGP_HIP(c, hipMemcpy(a->T, dt.p, sizeof(double) * mm, hipMemcpyDeviceToHost));
  if (a->snap && tap.nsnap > 0) ZIGP_HIP(c, hipMemcpy(a->snap, dsnap.p, sizeof(double) * mm * tap.nsnap, hipMemcpyDeviceToHost));
  if (a->facts) {
    a->facts[ZIGP_PSF_MP] = Mp; a->facts[ZIGP_PSF_NB] = nb; a->facts[ZIGP_PSF_LAUNCHES] = (int64_t)tap.rec.size() / PT_REC;
    a->facts[ZIGP_PSF_IMAGES] = tap.nsnap; a->facts[ZIGP_PSF_INFO] = h;
    for (int k = ZIGP_PSF_INFO + 1; k < ZIGP_PSF_REC; ++k) a->facts[k] = 0;
    std::copy(tap.rec.begin(), tap.rec.end(), a->facts + ZIGP_PSF_REC);
  }
  if (h != 0) {
    c->info = h;
    char b[256];
    snprintf(b, sizeof(b), "Cholesky decomposition was not successful for A: the input might not be positive definite (pivot %d)", h);
    c->err = b;
    return ZIGP_ENOTPD;
  }
  return 0;
}

// ---- stage diagnostics (include/zigp_diag.h): one chunk's stage on caller-supplied operands, through the chunk loop's own functions ----
namespace {
// host (rows x cols, row-major) -> device [rows_p][cols] with zero rows behind it
int stage_upload_rows(zigp_ctx* c, DevBuf& buf, const double* src, int64_t rows, int64_t rows_p, int64_t cols) {
  ZIGP_ENSURE(c, buf, (size_t)rows_p * cols);
  ZIGP_HIP(c, hipMemsetAsync(buf.p, 0, sizeof(double) * rows_p * cols, c->stream));
  if (src) ZIGP_HIP(c, hipMemcpyAsync(buf.p, src, sizeof(double) * rows * cols, hipMemcpyHostToDevice, c->stream));
  return 0;
}
// host (M,M) -> device (Mp,Mp), `pad` on the diagonal behind it
int stage_upload_square(zigp_ctx* c, DevBuf& buf, const double* src, int M, int Mp, double pad) {
  std::vector<double> h((size_t)Mp * Mp, 0.0);
  for (int i = 0; i < Mp; ++i) {
    if (i < M) memcpy(&h[(size_t)i * Mp], src + (size_t)i * M, sizeof(double) * M);
    else h[(size_t)i * Mp + i] = pad;
  }
  ZIGP_ENSURE(c, buf, h.size());
  ZIGP_HIP(c, hipMemcpyAsync(buf.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));     // h goes out of scope
  return 0;
}
int stage_download_rows(zigp_ctx* c, const double* dev, double* dst, int64_t rows, int64_t cols) {
  if (dst) ZIGP_HIP(c, hipMemcpyAsync(dst, dev, sizeof(double) * rows * cols, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
bool stage_chunk_ok(int64_t Nc) { return Nc >= 1024 && Nc % 1024 == 0 && Nc <= (1 << 20); }
}  // namespace

namespace {
int stage_chunk_forward(zigp_ctx* c, int64_t Nc, int32_t need_grad, int32_t only, const zigp_stage_latent* lat, int64_t* facts, Param par) {
  if (!c) return ZIGP_EARG;
  if (!lat || !facts || !stage_chunk_ok(Nc) || only < -1 || only > 1) return fail_arg(c, "zigp_test_chunk_forward: bad arguments");
  for (int h = 0; h < 2; ++h) {
    const zigp_stage_latent& q = lat[h];
    if (q.M <= 0) return fail_arg(c, "zigp_test_chunk_forward: M must be positive");
    if (only >= 0 && only != h) continue;
    if (!q.W || !q.v || !q.s2 || !q.K || (!q.A1 && !(is_white(par) && !need_grad)) || !q.part || (need_grad && (!q.Rt || !q.Jp)))
      return fail_arg(c, "zigp_test_chunk_forward: NULL operand of a latent that runs");
  }
  ZIGP_HIP(c, hipSetDevice(c->device));
  const bool grad = need_grad != 0, white = is_white(par);     // Diag or White: a WhiteFull chunk is Diag's launches (include/zigp_diag.h)
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const zigp_stage_latent& q = lat[h];
    lt.M = q.M; lt.Mp = (int)round_up(q.M, BM);
    const int Mp = lt.Mp;
    const size_t np = Mp / 32;
    const bool has_a1 = !white || grad;      // a whitened value-only / predict pass stores no A panel
    ZIGP_ENSURE(c, lt.Wt, (size_t)Mp * Mp); ZIGP_ENSURE(c, lt.vec, 4 * (size_t)Mp + 8); ZIGP_ENSURE(c, lt.wh, 4 * (size_t)Mp + 8);
    if (has_a1) ZIGP_ENSURE(c, lt.A1, (size_t)Mp * Nc);
    ZIGP_ENSURE(c, lt.part, 3 * np * Nc);
    if (grad) ZIGP_ENSURE(c, lt.Jp, (size_t)Mp * Nc);
    if (only >= 0 && only != h) {      // planned, not launched: only the buffers chunk_forward takes addresses of
      ZIGP_ENSURE(c, lt.W, (size_t)Mp * Mp); ZIGP_ENSURE(c, lt.s2, Mp); ZIGP_ENSURE(c, lt.K, (size_t)Mp * Nc); ZIGP_ENSURE(c, lt.Rt, (size_t)Mp * Mp);
      ZIGP_ENSURE(c, lt.Wp, (size_t)Mp * Mp);
      continue;
    }
    ZIGP_TRY(stage_upload_square(c, lt.W, q.W, q.M, Mp, 1.0));
    hipLaunchKernelGGL(k_transpose, dim3(Mp / 32, Mp / 32), dim3(32, 8), 0, c->stream, lt.W.p, (int64_t)Mp, lt.Wt.p);
    ZIGP_HIP(c, hipGetLastError());
    if (white) {      // the epilogue weights (Latent::wh: s2 = s^2 - 1, then v = u) and the J' factor image D W, zero padded
      if (grad) ZIGP_TRY(stage_upload_square(c, lt.Wp, q.Rt, q.M, Mp, 0.0));
      ZIGP_HIP(c, hipMemsetAsync(lt.wh.p, 0, sizeof(double) * (4 * (size_t)Mp + 8), c->stream));
      ZIGP_HIP(c, hipMemcpyAsync(lt.wh.p, q.s2, sizeof(double) * q.M, hipMemcpyHostToDevice, c->stream));
      ZIGP_HIP(c, hipMemcpyAsync(lt.wh.p + Mp, q.v, sizeof(double) * q.M, hipMemcpyHostToDevice, c->stream));
    } else {
      if (grad) ZIGP_TRY(stage_upload_square(c, lt.Rt, q.Rt, q.M, Mp, -1.0));
      ZIGP_TRY(stage_upload_rows(c, lt.s2, q.s2, q.M, Mp, 1));
      ZIGP_HIP(c, hipMemsetAsync(lt.vec.p, 0, sizeof(double) * (4 * (size_t)Mp + 8), c->stream));
      ZIGP_HIP(c, hipMemcpyAsync(lt.vec.p, q.v, sizeof(double) * q.M, hipMemcpyHostToDevice, c->stream));
    }
    ZIGP_TRY(stage_upload_rows(c, lt.K, q.K, q.M, Mp, Nc));
    if (has_a1) ZIGP_HIP(c, hipMemsetAsync(lt.A1.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * Mp * Nc, c->stream));
    if (grad) ZIGP_HIP(c, hipMemsetAsync(lt.Jp.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * Mp * Nc, c->stream));
    ZIGP_HIP(c, hipMemsetAsync(lt.part.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * 3 * np * Nc, c->stream));
  }
  const int M[2] = {lat[0].M, lat[1].M};
  ChunkPlan pl = chunk_plan(M, Nc, par, grad, c->trmm_tail, false);
  ZIGP_TRY(upload_plan(c, pl));
  if (only >= 0) { ChunkPlan::Lat& o = pl.lat[1 - only]; o.a1 = TileList(); o.a2j = TileList(); }
  if (white) {
    ZIGP_TRY(chunk_forward_white(c, pl, grad, false));
    if (grad) ZIGP_TRY(chunk_forward_white(c, pl, true, true));
  } else ZIGP_TRY(chunk_forward(c, pl, par, grad));
  for (int h = 0; h < 2; ++h) {
    if (only >= 0 && only != h) continue;
    Latent& lt = c->lat[h];
    if (!white || grad) ZIGP_TRY(stage_download_rows(c, lt.A1.p, lat[h].A1, lat[h].M, Nc));
    if (grad) ZIGP_TRY(stage_download_rows(c, lt.Jp.p, lat[h].Jp, lat[h].M, Nc));
    ZIGP_TRY(stage_download_rows(c, lt.part.p, lat[h].part, 3 * (int64_t)(lt.Mp / 32), Nc));
  }
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  zigp_params pp;
  memset(&pp, 0, sizeof(pp));
  DenseCall k;
  memset(static_cast<void*>(&k.hl), 0, sizeof(k.hl));
  k.p = &pp; k.dX = nullptr; k.dY = nullptr; k.Nrows = Nc; k.D = 1; k.jitter = 0; k.scale = 1; k.g_offset = 0; k.row_begin = 0; k.row_end = Nc;
  k.include_kl = 0; k.predict = false; k.d_out9 = nullptr; k.need_grad = grad; k.has_rows = true;
  const PwArgs a = dense_pointwise_args(c, k, 0, Nc);     // the row counts the point-wise stage is told
  facts[0] = pl.paired ? 1 : 0; facts[1] = pl.tail.units[0]; facts[2] = pl.tail.units[1]; facts[3] = c->lat[0].Mp; facts[4] = c->lat[1].Mp;
  facts[5] = a.np_f; facts[6] = a.np_g; facts[7] = a.np1_f; facts[8] = a.np2_f; facts[9] = a.np1_g; facts[10] = a.np2_g; facts[11] = 0;
  return ZIGP_OK;
}
}  // namespace
int zigp_test_chunk_forward(zigp_ctx* c, int64_t Nc, int32_t need_grad, int32_t only, const zigp_stage_latent* lat, int64_t* facts) {
  return stage_chunk_forward(c, Nc, need_grad, only, lat, facts, Param::Diag);
}
int zigp_test_chunk_forward_white(zigp_ctx* c, int64_t Nc, int32_t need_grad, int32_t only, const zigp_stage_latent* lat, int64_t* facts) {
  return stage_chunk_forward(c, Nc, need_grad, only, lat, facts, Param::White);
}

// ---- full-covariance M x M stage (zigp_set_q_full), one latent, through latent_qfull_stage / _factors / _dlq ----
namespace {
int stage_qfull_operands(zigp_ctx* c, Latent& lt, int M, const double* Lq, const double* u) {
  lt.M = M; lt.Mp = (int)round_up(M, BM);
  const size_t Mp = lt.Mp, mm = (size_t)M * M;
  ZIGP_ENSURE(c, lt.Lraw, mm); ZIGP_ENSURE(c, lt.Lq, Mp * Mp); ZIGP_ENSURE(c, lt.lqssq, Mp * Mp / 256); ZIGP_ENSURE(c, lt.wh, 4 * Mp + 8);
  ZIGP_HIP(c, hipMemcpyAsync(lt.Lraw.p, Lq, sizeof(double) * mm, hipMemcpyHostToDevice, c->stream));
  ZIGP_TRY(stage_upload_rows(c, lt.u, u, M, (int64_t)Mp, 1));
  return latent_qfull_stage(c, lt);
}
int stage_download_square(zigp_ctx* c, const double* dev, int M, int Mp, double* dst) {
  if (!dst) return 0;
  std::vector<double> h((size_t)Mp * Mp);
  ZIGP_HIP(c, hipMemcpyAsync(h.data(), dev, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < M; ++i) memcpy(dst + (size_t)i * M, &h[(size_t)i * Mp], sizeof(double) * M);
  return 0;
}
}  // namespace
int zigp_test_q_full_forward(zigp_ctx* c, int32_t M, const double* W, const double* Lq, const double* u, double* TmI, double* Rt, double* kl) {
  if (!c) return ZIGP_EARG;
  if (M <= 0 || !W || !Lq || !u) return fail_arg(c, "zigp_test_q_full_forward: bad arguments");
  for (int m = 0; m < M; ++m)
    if (!(Lq[(size_t)m * M + m] != 0)) return fail_arg(c, "zigp_test_q_full_forward: zero diagonal entry of Lq");
  ZIGP_HIP(c, hipSetDevice(c->device));
  Latent& lt = c->lat[0];
  ZIGP_TRY(stage_qfull_operands(c, lt, M, Lq, u));
  const int Mp = lt.Mp;
  ZIGP_TRY(stage_upload_square(c, lt.W, W, M, Mp, 1.0));
  ZIGP_ENSURE(c, lt.P, (size_t)Mp * Mp); ZIGP_ENSURE(c, lt.Rt, (size_t)Mp * Mp);
  ZIGP_HIP(c, hipMemsetAsync(lt.P.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * Mp * Mp, c->stream));
  ZIGP_HIP(c, hipMemsetAsync(lt.Rt.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * Mp * Mp, c->stream));
  ZIGP_TRY(latent_qfull_factors(c, lt));
  ZIGP_TRY(stage_download_square(c, lt.P.p, M, Mp, TmI));
  ZIGP_TRY(stage_download_square(c, lt.Rt.p, M, Mp, Rt));
  if (kl) ZIGP_HIP(c, hipMemcpyAsync(kl, lt.wh.p + 3 * (size_t)Mp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}
int zigp_test_q_full_dlq(zigp_ctx* c, int32_t M, const double* C1, const double* Lq, int32_t include_kl, double* dLq) {
  if (!c) return ZIGP_EARG;
  if (M <= 0 || !C1 || !Lq || !dLq) return fail_arg(c, "zigp_test_q_full_dlq: bad arguments");
  for (int m = 0; m < M; ++m)
    if (!(Lq[(size_t)m * M + m] != 0)) return fail_arg(c, "zigp_test_q_full_dlq: zero diagonal entry of Lq");
  ZIGP_HIP(c, hipSetDevice(c->device));
  Latent& lt = c->lat[0];
  ZIGP_TRY(stage_qfull_operands(c, lt, M, Lq, nullptr));
  const int Mp = lt.Mp;
  ZIGP_TRY(stage_upload_square(c, lt.T1, C1, M, Mp, 0.0));
  ZIGP_ENSURE(c, lt.dLq, (size_t)Mp * Mp);
  ZIGP_HIP(c, hipMemsetAsync(lt.dLq.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * Mp * Mp, c->stream));
  ZIGP_TRY(latent_qfull_dlq(c, lt, true, include_kl != 0));
  ZIGP_TRY(stage_download_square(c, lt.dLq.p, M, Mp, dLq));
  return ZIGP_OK;
}

int zigp_test_latents_forward(zigp_ctx* c, const zigp_params* p, double jitter, int32_t need_grad, double* const* out_f, double* const* out_g) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  if (!out_f || !out_g || !(jitter >= 0)) return fail_arg(c, "zigp_test_latents_forward: bad arguments");
  if (c->q_full) return fail_arg(c, "zigp_test_latents_forward: the diagonal stages only (zigp_set_q_full is on; see zigp_test_q_full_forward)");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const Param par = param_of(c);     // Diag or White: a full-covariance context was refused above
  const bool white = is_white(par), grad = need_grad != 0;
  HostLatent hl[2] = {{p->Mf, p->Zf, p->u_fm, p->u_fs_sqrt, p->ell_f, p->var_f}, {p->Mg, p->Zg, p->u_gm, p->u_gs_sqrt, p->ell_g, p->var_g}};
  ZIGP_TRY(begin_staged_call(c));
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  ZIGP_TRY(latents_upload(c, hl, p->D, par));
  ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
  ZIGP_TRY(latents_forward(c, hl, p->D, jitter, par, true, grad, nullptr, nullptr));
  ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  ZIGP_TRY(check_info(c, "Kuu"));
  double* const* outs[2] = {out_f, out_g};
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const int M = lt.M, Mp = lt.Mp;
    double* const* o = outs[h];
    // (M,M) images; one the mode or need_grad does not produce is left untouched
    const double* mats[ZIGP_FWD_OUTS] = {nullptr};
    mats[ZIGP_FWD_W] = lt.W.p; mats[ZIGP_FWD_L] = lt.L.p; mats[ZIGP_FWD_KUU] = lt.Kuu.p; mats[ZIGP_FWD_WT] = lt.Wt.p;
    if (grad) mats[ZIGP_FWD_WP] = lt.Wp.p;
    if (grad && !white) { mats[ZIGP_FWD_RT] = lt.Rt.p; mats[ZIGP_FWD_P] = lt.P.p; mats[ZIGP_FWD_QT] = lt.Qt.p; }
    for (int q = 0; q < ZIGP_FWD_OUTS; ++q)
      if (mats[q]) ZIGP_TRY(stage_download_square(c, mats[q], M, Mp, o[q]));
    const double* vec = lt.vec.p;
    if (!white) {
      ZIGP_TRY(stage_download_rows(c, vec, o[ZIGP_FWD_V], 1, M));
      ZIGP_TRY(stage_download_rows(c, vec + Mp, o[ZIGP_FWD_ALPHA], 1, M));
      ZIGP_TRY(stage_download_rows(c, vec + 2 * Mp, o[ZIGP_FWD_DKINV], 1, M));
      ZIGP_TRY(stage_download_rows(c, vec + 3 * Mp, o[ZIGP_FWD_KL], 1, 1));
    } else {
      if (grad) ZIGP_TRY(stage_download_rows(c, vec + Mp, o[ZIGP_FWD_ALPHA], 1, M));
      ZIGP_TRY(stage_download_rows(c, lt.wh.p + 3 * Mp, o[ZIGP_FWD_KL], 1, 1));
      if (o[ZIGP_FWD_WH])
        for (int q = 0; q < 3; ++q) ZIGP_TRY(stage_download_rows(c, lt.wh.p + (size_t)q * Mp, o[ZIGP_FWD_WH] + (size_t)q * M, 1, M));
    }
    ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  }
  prof_collect(c);
  return ZIGP_OK;
}

namespace {
// lik != 0: the head's kernel (zigp_test_pointwise_head) -- the g planes and their counts are not read, the predict block has four rows
int stage_pointwise(zigp_ctx* c, const zigp_stage_pointwise* s, Param par, int lik = 0) {
  if (!c) return ZIGP_EARG;
  if (lik != 0 && lik != ZIGP_LIK_GAUSSIAN && lik != ZIGP_LIK_BERNOULLI)
    return fail_arg(c, "zigp_test_pointwise_head: lik must be ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI");
  if (!s || s->mode < 0 || s->mode > 2 || s->repeat < 1 || !stage_chunk_ok(s->Nc) || !s->part_f || (!lik && !s->part_g) || !s->acc)
    return fail_arg(c, "zigp_test_pointwise: bad arguments");
  if (s->np_f < 1 || s->np1_f < 0 || s->np2_f < 0 || s->np1_f > s->np_f || s->np2_f > s->np_f ||
      (!lik && (s->np_g < 1 || s->np1_g < 0 || s->np2_g < 0 || s->np1_g > s->np_g || s->np2_g > s->np_g)))
    return fail_arg(c, "zigp_test_pointwise: need 0 <= np1, np2 <= np");
  if (s->D < 1 || s->D > ZIGP_MAX_D || (s->D > MAXD && s->mean_on) || !s->X || s->Nrows <= 0 || s->n0 < 0 || s->row_end < s->n0 || s->row_end > s->Nrows || s->row_end > s->n0 + s->Nc)
    return fail_arg(c, "zigp_test_pointwise: need X (Nrows,D), 1 <= D <= " ZIGP_MAX_D_STR " (a mean function: D <= 8) and n0 <= row_end <= min(Nrows, n0 + Nc)");
  if (s->mode == 1 && (!s->gm_f || !s->gv_f || !s->gm_g || !s->gv_g)) return fail_arg(c, "zigp_test_pointwise: gradient mode needs gm / gv outputs");
  if (s->mode == 2 ? !s->out9 : !s->Y) return fail_arg(c, "zigp_test_pointwise: predict needs out9, the ELBO modes need Y");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int64_t Nc = s->Nc;
  const size_t nacc = (size_t)(Nc / PW_PTS) * PW_ACC;
  DevBuf dx, dy, pf, pg;
  ZIGP_TRY(stage_upload_rows(c, dx, s->X, s->Nrows, s->Nrows, s->D));
  if (s->Y) ZIGP_TRY(stage_upload_rows(c, dy, s->Y, s->Nrows, s->Nrows, 1));
  ZIGP_TRY(stage_upload_rows(c, pf, s->part_f, 3 * (int64_t)s->np_f, 3 * (int64_t)s->np_f, Nc));
  if (!lik) ZIGP_TRY(stage_upload_rows(c, pg, s->part_g, 3 * (int64_t)s->np_g, 3 * (int64_t)s->np_g, Nc));
  ZIGP_TRY(stage_upload_rows(c, c->pw_part, s->acc, (int64_t)nacc, (int64_t)nacc, 1));
  for (int h = 0; h < 2; ++h) { ZIGP_ENSURE(c, c->lat[h].gm, Nc); ZIGP_ENSURE(c, c->lat[h].gv, Nc); }
  if (s->mode == 2) { ZIGP_ENSURE(c, c->out9, (size_t)9 * s->row_end + 1); ZIGP_HIP(c, hipMemsetAsync(c->out9.p, 0, sizeof(double) * (9 * s->row_end + 1), c->stream)); }
  zigp_params pp;
  memset(&pp, 0, sizeof(pp));
  pp.var_f = s->var_f; pp.var_g = s->var_g; pp.noise = s->noise;
  DenseCall k;
  memset(static_cast<void*>(&k.hl), 0, sizeof(k.hl));
  k.p = &pp; k.dX = dx.p; k.dY = s->Y ? dy.p : nullptr; k.Nrows = s->Nrows; k.D = s->D; k.jitter = 0; k.scale = s->scale; k.g_offset = s->g_offset;
  k.row_begin = 0; k.row_end = s->row_end; k.include_kl = 0; k.predict = s->mode == 2; k.d_out9 = s->mode == 2 ? c->out9.p : nullptr;
  k.need_grad = s->mode == 1; k.has_rows = true;
  // the context's mean function for the duration of the call
  const bool mean_on = c->mean_on; const double mean_b = c->mean_b; double mean_a[MAXD];
  for (int d = 0; d < MAXD; ++d) { mean_a[d] = c->mean_a[d]; c->mean_a[d] = s->mean_a[d]; }
  c->mean_on = s->mean_on != 0; c->mean_b = s->mean_b;
  PwArgs a = dense_pointwise_args(c, k, s->n0, Nc);
  c->mean_on = mean_on; c->mean_b = mean_b;
  for (int d = 0; d < MAXD; ++d) c->mean_a[d] = mean_a[d];
  a.part_f = pf.p; a.part_g = pg.p; a.np_f = s->np_f; a.np_g = s->np_g;
  a.np1_f = s->np1_f; a.np2_f = s->np2_f; a.np1_g = s->np1_g; a.np2_g = s->np2_g;
  for (int r = 0; r < s->repeat; ++r) ZIGP_TRY(dense_pointwise_launch(c, par, k.predict, k.need_grad, a, nullptr, lik));
  if (s->mode == 1) {
    ZIGP_TRY(stage_download_rows(c, c->lat[0].gm.p, s->gm_f, 1, Nc)); ZIGP_TRY(stage_download_rows(c, c->lat[0].gv.p, s->gv_f, 1, Nc));
    ZIGP_TRY(stage_download_rows(c, c->lat[1].gm.p, s->gm_g, 1, Nc)); ZIGP_TRY(stage_download_rows(c, c->lat[1].gv.p, s->gv_g, 1, Nc));
  }
  if (s->mode == 2) ZIGP_TRY(stage_download_rows(c, c->out9.p, s->out9, lik ? 4 : 9, s->row_end));
  else ZIGP_TRY(stage_download_rows(c, c->pw_part.p, s->acc, 1, (int64_t)nacc));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}
}  // namespace
int zigp_test_pointwise(zigp_ctx* c, const zigp_stage_pointwise* s) { return stage_pointwise(c, s, Param::Diag); }
int zigp_test_pointwise_white(zigp_ctx* c, const zigp_stage_pointwise* s) { return stage_pointwise(c, s, Param::White); }
int zigp_test_pointwise_head(zigp_ctx* c, int32_t lik, int32_t white, const zigp_stage_pointwise* s) {
  if (!c) return ZIGP_EARG;
  if (lik != ZIGP_LIK_GAUSSIAN && lik != ZIGP_LIK_BERNOULLI) return fail_arg(c, "zigp_test_pointwise_head: lik must be ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI");
  return stage_pointwise(c, s, white ? Param::White : Param::Diag, lik);
}

int zigp_test_kgrad(zigp_ctx* c, int32_t M, int32_t D, int64_t Nc, int64_t Nrows, int64_t n0, const double* Jp, const double* K, const double* alpha,
                    const double* gm, const double* gv, const double* X, const double* Z, const double* ell, const double* centre, int32_t exact,
                    double* krow) {
  if (!c) return ZIGP_EARG;
  if (M <= 0 || D < 1 || D > ZIGP_MAX_D || !stage_chunk_ok(Nc) || Nrows <= 0 || n0 < 0 || n0 >= Nrows || !Jp || !K || !alpha || !gm || !gv || !X || !Z || !krow ||
      exact < -1 || exact > 1 || (exact < 0 && !ell))
    return fail_arg(c, "zigp_test_kgrad: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  Latent& lt = c->lat[0];
  lt.M = M; lt.Mp = (int)round_up(M, BM);
  const int Mp = lt.Mp, Wd = 2 + 2 * D;
  if (exact < 0 || !centre) {
    double one[WIDE_MAXD];
    for (double& v : one) v = 1.0;
    kgrad_centre(lt, Z, ell ? ell : one, M, D);
  }
  if (exact >= 0) lt.kg_exact = exact != 0;
  if (centre) for (int d = 0; d < WIDE_MAXD; ++d) lt.zc[d] = d < D ? centre[d] : 0.0;
  DevBuf dx;
  ZIGP_TRY(stage_upload_rows(c, dx, X, Nrows, Nrows, D));
  ZIGP_TRY(stage_upload_rows(c, lt.Z, Z, M, Mp, D));
  ZIGP_TRY(stage_upload_rows(c, lt.K, K, M, Mp, Nc));
  ZIGP_TRY(stage_upload_rows(c, lt.Jp, Jp, M, Mp, Nc));
  if (D > MAXD && Mp > M)      // the wide forms must not read the padded rows of J': they hold the stage sentinel here
    ZIGP_HIP(c, hipMemsetAsync(lt.Jp.p + (size_t)M * Nc, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * (size_t)(Mp - M) * Nc, c->stream));
  ZIGP_TRY(stage_upload_rows(c, lt.gm, gm, 1, 1, Nc));
  ZIGP_TRY(stage_upload_rows(c, lt.gv, gv, 1, 1, Nc));
  ZIGP_ENSURE(c, lt.vec, 4 * (size_t)Mp + 8);
  ZIGP_HIP(c, hipMemsetAsync(lt.vec.p, 0, sizeof(double) * (4 * (size_t)Mp + 8), c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(lt.vec.p + Mp, alpha, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
  ZIGP_ENSURE(c, lt.krow, (size_t)KG_SPLIT * Mp * Wd);
  ZIGP_HIP(c, hipMemsetAsync(lt.krow.p, 0, sizeof(double) * KG_SPLIT * Mp * Wd, c->stream));
  for (int sp = 0; sp < KG_SPLIT; ++sp)
    ZIGP_HIP(c, hipMemcpyAsync(lt.krow.p + (size_t)sp * Mp * Wd, krow + (size_t)sp * M * Wd, sizeof(double) * M * Wd, hipMemcpyHostToDevice, c->stream));
  TileList mom;
  if (D > MAXD && !lt.kg_exact) {
    ZIGP_TRY(ensure_kgrad_wide(c, lt, Nc));
    ZIGP_TRY(get_tiles(c, kgmom_tiles(Mp / BM, Nc), mom));
  }
  ZIGP_TRY(latent_chunk_kgrad(c, lt, dx.p, Nrows, n0, Nc, D, ell, mom));
  for (int sp = 0; sp < KG_SPLIT; ++sp)
    ZIGP_HIP(c, hipMemcpyAsync(krow + (size_t)sp * M * Wd, lt.krow.p + (size_t)sp * Mp * Wd, sizeof(double) * M * Wd, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_test_kgrad_kind(zigp_ctx* c, int32_t kind, int32_t M, int32_t D, int64_t Nc, int64_t Nrows, int64_t n0, const double* Jp, const double* K,
                         const double* Kd, const double* alpha, const double* gm, const double* gv, const double* X, const double* Z, double* krow) {
  if (!c) return ZIGP_EARG;
  if (kind == ZIGP_KERN_RBF) return zigp_test_kgrad(c, M, D, Nc, Nrows, n0, Jp, K, alpha, gm, gv, X, Z, nullptr, nullptr, 1, krow);
  if (kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52) return fail_arg(c, "zigp_test_kgrad_kind: unknown kernel kind");
  if (M <= 0 || D < 1 || D > MAXD || !stage_chunk_ok(Nc) || Nrows <= 0 || n0 < 0 || n0 >= Nrows || !Jp || !K || !Kd || !alpha || !gm || !gv || !X || !Z || !krow)
    return fail_arg(c, "zigp_test_kgrad_kind: bad arguments (a Matern kind needs 1 <= D <= 8 and the K' panel)");
  ZIGP_HIP(c, hipSetDevice(c->device));
  Latent lt;      // a latent of this call's own: the context's panels stay as they are
  lt.M = M; lt.Mp = (int)round_up(M, BM);
  const int Mp = lt.Mp, Wd = 2 + 2 * D;
  DevBuf dx;
  ZIGP_TRY(stage_upload_rows(c, dx, X, Nrows, Nrows, D));
  ZIGP_TRY(stage_upload_rows(c, lt.Z, Z, M, Mp, D));
  ZIGP_TRY(stage_upload_rows(c, lt.K, K, M, Mp, Nc));
  ZIGP_TRY(stage_upload_rows(c, lt.Kd, Kd, M, Mp, Nc));
  ZIGP_TRY(stage_upload_rows(c, lt.Jp, Jp, M, Mp, Nc));
  ZIGP_TRY(stage_upload_rows(c, lt.gm, gm, 1, 1, Nc));
  ZIGP_TRY(stage_upload_rows(c, lt.gv, gv, 1, 1, Nc));
  ZIGP_ENSURE(c, lt.vec, 4 * (size_t)Mp + 8);
  ZIGP_HIP(c, hipMemsetAsync(lt.vec.p, 0, sizeof(double) * (4 * (size_t)Mp + 8), c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(lt.vec.p + Mp, alpha, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
  ZIGP_ENSURE(c, lt.krow, (size_t)KG_SPLIT * Mp * Wd);
  ZIGP_HIP(c, hipMemsetAsync(lt.krow.p, 0, sizeof(double) * KG_SPLIT * Mp * Wd, c->stream));
  for (int sp = 0; sp < KG_SPLIT; ++sp)
    ZIGP_HIP(c, hipMemcpyAsync(lt.krow.p + (size_t)sp * Mp * Wd, krow + (size_t)sp * M * Wd, sizeof(double) * M * Wd, hipMemcpyHostToDevice, c->stream));
  ZIGP_TRY(latent_chunk_kgrad(c, lt, dx.p, Nrows, n0, Nc, D, nullptr, TileList(), kind));
  for (int sp = 0; sp < KG_SPLIT; ++sp)
    ZIGP_HIP(c, hipMemcpyAsync(krow + (size_t)sp * M * Wd, lt.krow.p + (size_t)sp * Mp * Wd, sizeof(double) * M * Wd, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_test_rank_update(zigp_ctx* c, int32_t M, int32_t nchunks, const int64_t* Nc, const double* const* A1, const double* const* gv, double* C1,
                          int64_t* plan) {
  if (!c) return ZIGP_EARG;
  if (M <= 0 || nchunks < 1 || !Nc || !A1 || !gv || !C1 || !plan) return fail_arg(c, "zigp_test_rank_update: bad arguments");
  int64_t Nmax = 0;
  for (int i = 0; i < nchunks; ++i) {
    if (!stage_chunk_ok(Nc[i]) || !A1[i] || !gv[i]) return fail_arg(c, "zigp_test_rank_update: every chunk needs A1, gv and a multiple of 1024 rows");
    Nmax = std::max(Nmax, Nc[i]);
  }
  ZIGP_HIP(c, hipSetDevice(c->device));
  Latent& lt = c->lat[0];
  lt.M = M; lt.Mp = (int)round_up(M, BM);
  const int Mp = lt.Mp;
  const size_t mm = (size_t)Mp * Mp;
  const SyrPlan sp = syr_plan(Mp / BM);
  ZIGP_ENSURE(c, lt.dLpart, (size_t)sp.planes() * mm); ZIGP_ENSURE(c, lt.T1, mm);
  ZIGP_ENSURE(c, lt.A1, (size_t)Mp * Nmax); ZIGP_ENSURE(c, lt.gv, Nmax);
  ZIGP_HIP(c, hipMemsetAsync(lt.dLpart.p, 0, sizeof(double) * sp.planes() * mm, c->stream));
  ZIGP_HIP(c, hipMemsetAsync(lt.T1.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * mm, c->stream));
  const int Ms[2] = {M, M};
  for (int i = 0; i < nchunks; ++i) {
    ChunkPlan pl = chunk_plan(Ms, Nc[i], Param::Diag, true, c->trmm_tail, false);
    ZIGP_TRY(upload_plan(c, pl));
    ZIGP_TRY(stage_upload_rows(c, lt.A1, A1[i], M, Mp, Nc[i]));
    ZIGP_TRY(stage_upload_rows(c, lt.gv, gv[i], 1, 1, Nc[i]));
    ZIGP_TRY(latent_chunk_syrk(c, pl, 0));
  }
  latent_sym_from_planes(c, lt);
  ZIGP_HIP(c, hipGetLastError());
  std::vector<double> hc(mm);
  ZIGP_HIP(c, hipMemcpyAsync(hc.data(), lt.T1.p, sizeof(double) * mm, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < M; ++i) memcpy(C1 + (size_t)i * M, &hc[(size_t)i * Mp], sizeof(double) * M);
  plan[0] = sp.So; plan[1] = sp.Sd;
  return ZIGP_OK;
}

// ---- M x M reverse stage of one latent (include/zigp_diag.h), through latent_mxm_backward ----
namespace {
// host (rows x cols) -> device (rows_p x cols_p), `pad` outside the real block; lower: entries above the diagonal are zero
int stage_upload_padded(zigp_ctx* c, DevBuf& buf, const double* src, int rows, int cols, int rows_p, int cols_p, double pad, bool lower = false) {
  std::vector<double> h((size_t)rows_p * cols_p, pad);
  for (int i = 0; i < rows; ++i) memcpy(&h[(size_t)i * cols_p], src + (size_t)i * cols, sizeof(double) * cols);
  if (lower)
    for (int i = 0; i < rows_p; ++i)
      for (int j = i + 1; j < cols_p; ++j) h[(size_t)i * cols_p + j] = 0.0;
  ZIGP_ENSURE(c, buf, h.size());
  ZIGP_HIP(c, hipMemcpyAsync(buf.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));     // h goes out of scope
  return 0;
}
}  // namespace
int zigp_test_mxm_backward(zigp_ctx* c, const zigp_stage_mxm* a) {
  if (!c) return ZIGP_EARG;
  if (!a) return fail_arg(c, "zigp_test_mxm_backward: NULL arguments");
  if (a->M <= 0) return fail_arg(c, "zigp_test_mxm_backward: M must be positive");
  if (a->D < 1 || a->D > ZIGP_MAX_D) return fail_arg(c, "zigp_test_mxm_backward: D must be in [1, " ZIGP_MAX_D_STR "] (ZIGP_MAX_D)");
  if (a->mode < 0 || a->mode > 2) return fail_arg(c, "zigp_test_mxm_backward: mode must be 0 (unwhitened), 1 (whitened diagonal) or 2 (whitened full covariance)");
  if (!(a->jitter >= 0) || !(a->pad == a->pad)) return fail_arg(c, "zigp_test_mxm_backward: jitter must be >= 0 and pad a number");
  if (!a->W || !a->L || !a->Kuu || !a->Z || !a->s || !a->alpha || !a->krow || (a->mode == 0 && !a->v) || (a->with_data && !a->C1))
    return fail_arg(c, "zigp_test_mxm_backward: NULL operand of the mode");
  const int M = a->M, D = a->D, Wd = 2 + 2 * D;
  const Param par = (Param)a->mode;
  const bool white = is_white(par), with_data = a->with_data != 0, with_kl = a->with_kl != 0;
  for (int m = 0; m < M; ++m)
    if (!((is_full(par) ? a->s[(size_t)m * M + m] : a->s[m]) != 0))
      return fail_arg(c, is_full(par) ? "zigp_test_mxm_backward: zero (or NaN) diagonal entry of Lq" : "zigp_test_mxm_backward: zero (or NaN) entry of s");
  ZIGP_HIP(c, hipSetDevice(c->device));
  Latent& lt = c->lat[0];
  lt.M = M; lt.Mp = (int)round_up(M, BM);
  if (c->lat[1].Mp <= 0) { c->lat[1].M = 1; c->lat[1].Mp = BM; }     // the zeroing path below walks both latents
  const int Mp = lt.Mp;
  const size_t mm = (size_t)Mp * Mp;
  // the call's accumulators, as a gradient step sizes and zeroes them (a1gm, du, dsq, krow; the rank-update planes when there are rows)
  {
    zigp_params pp;
    memset(&pp, 0, sizeof(pp));
    DenseCall k;
    memset(static_cast<void*>(&k.hl), 0, sizeof(k.hl));
    k.p = &pp; k.dX = nullptr; k.dY = nullptr; k.Nrows = 1024; k.D = D; k.jitter = a->jitter; k.scale = 1; k.g_offset = 0; k.row_begin = 0;
    k.row_end = with_data ? 1024 : 0; k.include_kl = with_kl ? 1 : 0; k.predict = false; k.d_out9 = nullptr; k.need_grad = true; k.has_rows = with_data;
    k.par = par; k.Nc = 1024;
    ZIGP_TRY(dense_prepare_buffers(c, k));
  }
  // operands
  ZIGP_TRY(stage_upload_square(c, lt.W, a->W, M, Mp, 1.0));
  ZIGP_TRY(stage_upload_square(c, lt.L, a->L, M, Mp, 1.0));
  ZIGP_TRY(stage_upload_padded(c, lt.Kuu, a->Kuu, M, M, Mp, Mp, a->pad));
  ZIGP_TRY(stage_upload_padded(c, lt.Z, a->Z, M, D, Mp, D, a->pad));
  ZIGP_ENSURE(c, lt.vec, 4 * (size_t)Mp + 8);
  ZIGP_HIP(c, hipMemsetAsync(lt.vec.p, 0, sizeof(double) * (4 * (size_t)Mp + 8), c->stream));
  if (a->v) ZIGP_HIP(c, hipMemcpyAsync(lt.vec.p, a->v, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemcpyAsync(lt.vec.p + Mp, a->alpha, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
  ZIGP_ENSURE(c, lt.Wp, mm);
  const dim3 gridmm(ceil_div((int64_t)mm, 256));
  lt.P_ready = false;
  if (is_full(par)) {          // the staged factor and its small vectors, then T - I -> P and R^T -> Rt
    ZIGP_TRY(stage_qfull_operands(c, lt, M, a->s, a->u));
    ZIGP_ENSURE(c, lt.P, mm); ZIGP_ENSURE(c, lt.Rt, mm);
    ZIGP_TRY(latent_qfull_factors(c, lt));
  } else if (white) {    // the whitened vectors (k_kl_white), then D W -> Wp
    ZIGP_TRY(stage_upload_padded(c, lt.u, a->u, a->u ? M : 0, 1, Mp, 1, 0.0));
    ZIGP_TRY(stage_upload_padded(c, lt.s, a->s, M, 1, Mp, 1, a->pad));
    ZIGP_ENSURE(c, lt.wh, 4 * (size_t)Mp + 8);
    hipLaunchKernelGGL(k_kl_white, dim3(1), dim3(256), 0, c->stream, lt.u.p, lt.s.p, lt.M, (int64_t)Mp, lt.wh.p);
    hipLaunchKernelGGL(k_rowscale, gridmm, dim3(256), 0, c->stream, lt.W.p, lt.wh.p, (int64_t)Mp, lt.Wp.p);
    ZIGP_HIP(c, hipGetLastError());
  } else {               // s^2 (one multiplication per entry, k_kuu_setup's), then W diag(s^2) -> Wp
    std::vector<double> s2(M);
    for (int m = 0; m < M; ++m) s2[m] = a->s[m] * a->s[m];
    ZIGP_TRY(stage_upload_padded(c, lt.s2, s2.data(), M, 1, Mp, 1, a->pad * a->pad));
    hipLaunchKernelGGL(k_colscale, gridmm, dim3(256), 0, c->stream, lt.W.p, lt.s2.p, (int64_t)Mp, lt.Wp.p);
    ZIGP_HIP(c, hipGetLastError());
    if (a->P) { ZIGP_TRY(stage_upload_square(c, lt.P, a->P, M, Mp, 1.0)); lt.P_ready = true; }
  }
  if (with_data) ZIGP_TRY(stage_upload_padded(c, lt.dLpart, a->C1, M, M, Mp, Mp, a->pad, true));     // plane 0; the others keep the step's zeros
  ZIGP_HIP(c, hipMemcpyAsync(lt.krow.p, a->krow, sizeof(double) * KG_SPLIT * Mp * Wd, hipMemcpyHostToDevice, c->stream));
  // scratch: whatever a launch reads before the stage wrote it shows
  ZIGP_ENSURE(c, lt.T1, mm); ZIGP_ENSURE(c, lt.T2, mm); ZIGP_ENSURE(c, lt.T3, mm);
  if (!white) ZIGP_ENSURE(c, lt.G, mm);
  for (double* q : {lt.T1.p, lt.T2.p, lt.T3.p, white ? (double*)nullptr : lt.G.p})
    if (q) ZIGP_HIP(c, hipMemsetAsync(q, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * mm, c->stream));
  if (is_full(par)) {
    ZIGP_ENSURE(c, lt.dLq, mm);
    ZIGP_HIP(c, hipMemsetAsync(lt.dLq.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * mm, c->stream));
  }
  const MxmTap tap = [&](int id, const double* dev) -> int {
    if (id < 0 || id >= ZIGP_MXM_TAPS || !a->tap[id]) return 0;
    return stage_download_square(c, dev, M, Mp, a->tap[id]);
  };
  const int rc = latent_mxm_backward(c, lt, D, a->jitter, par, with_data, with_kl, tap);
  lt.P_ready = false;
  ZIGP_TRY(rc);
  ZIGP_TRY(stage_download_rows(c, lt.a1gm.p, a->a1gm, 1, M));
  ZIGP_TRY(stage_download_rows(c, lt.du.p, a->du, 1, M));
  ZIGP_TRY(stage_download_rows(c, lt.dsq.p, a->dsq, 1, M));
  ZIGP_TRY(stage_download_rows(c, lt.krow.p, a->krow, (int64_t)KG_SPLIT * Mp, Wd));
  ZIGP_TRY(stage_download_square(c, lt.T3.p, M, Mp, a->G));
  if (is_full(par)) ZIGP_TRY(stage_download_square(c, lt.dLq.p, M, Mp, a->dLq));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

// ---- the result vector (k_dense_pack, k_pack_square) from caller-supplied accumulators, through dense_pack ----
int zigp_test_dense_pack(zigp_ctx* c, const zigp_stage_pack* a) {
  if (!c) return ZIGP_EARG;
  if (!a || !a->out) return fail_arg(c, "zigp_test_dense_pack: NULL arguments");
  if (a->D < 1 || a->D > ZIGP_MAX_D) return fail_arg(c, "zigp_test_dense_pack: D must be in [1, " ZIGP_MAX_D_STR "] (ZIGP_MAX_D)");
  if (a->mode < 0 || a->mode > 2 || a->pw_blocks < 1 || !a->pw) return fail_arg(c, "zigp_test_dense_pack: need a mode in 0 .. 2 and pw [pw_blocks][13], pw_blocks >= 1");
  if (a->mean_on && a->D > MAXD) return fail_arg(c, "zigp_test_dense_pack: the mean function's sums cover D <= 8");
  const int D = a->D, Wd = 2 + 2 * D;
  const Param par = (Param)a->mode;
  const bool grad = a->need_grad != 0, white = is_white(par), lq = is_full(par);     // lq: the latents carry a full factor (dLq, no dsq / s)
  size_t need = DP_HDR;
  for (int h = 0; h < 2; ++h) {
    const zigp_stage_pack_latent& q = a->lat[h];
    if (q.M <= 0) return fail_arg(c, "zigp_test_dense_pack: M must be positive");
    if (!q.kl_vec1 || (!lq && !q.kl_vec2)) return fail_arg(c, "zigp_test_dense_pack: NULL operand");
    if (grad && (!q.krow || !q.du || !q.ell || !(q.var > 0) || (lq ? !q.dLq : (!q.dsq || !q.s))))
      return fail_arg(c, "zigp_test_dense_pack: NULL operand of a gradient call (or var <= 0)");
    if (grad && !lq)
      for (int m = 0; m < q.M; ++m)
        if (!(q.s[m] != 0)) return fail_arg(c, "zigp_test_dense_pack: zero (or NaN) entry of s");
    if (grad) need += (size_t)q.M * D + q.M + (lq ? (size_t)q.M * q.M : (size_t)q.M) + D;
  }
  if (a->n_out != (int64_t)need) return fail_arg(c, "zigp_test_dense_pack: n_out must be 16 + sum over the latents of M D + M + (M or M M) + D (16 without need_grad)");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const size_t nacc = (size_t)a->pw_blocks * PW_ACC;
  ZIGP_TRY(stage_upload_rows(c, c->pw_part, a->pw, (int64_t)nacc, (int64_t)nacc, 1));
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const zigp_stage_pack_latent& q = a->lat[h];
    lt.M = q.M; lt.Mp = (int)round_up(q.M, BM); lt.var = q.var;
    const int M = lt.M, Mp = lt.Mp;
    // the small vectors in the layout k_dense_pack reads: [. | dKL/du | diagonal factor of dKL/ds | KL]
    DevBuf& vec = white ? lt.wh : lt.vec;
    ZIGP_ENSURE(c, vec, 4 * (size_t)Mp + 8);
    ZIGP_HIP(c, hipMemsetAsync(vec.p, 0, sizeof(double) * (4 * (size_t)Mp + 8), c->stream));
    ZIGP_HIP(c, hipMemcpyAsync(vec.p + Mp, q.kl_vec1, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    if (q.kl_vec2) ZIGP_HIP(c, hipMemcpyAsync(vec.p + 2 * (size_t)Mp, q.kl_vec2, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    ZIGP_HIP(c, hipMemcpyAsync(vec.p + 3 * (size_t)Mp, &q.kl, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (!grad) continue;
    ZIGP_ENSURE(c, lt.krow, (size_t)KG_SPLIT * Mp * Wd);
    ZIGP_HIP(c, hipMemsetAsync(lt.krow.p, 0, sizeof(double) * KG_SPLIT * Mp * Wd, c->stream));
    for (int sp = 0; sp < KG_SPLIT; ++sp)
      ZIGP_HIP(c, hipMemcpyAsync(lt.krow.p + (size_t)sp * Mp * Wd, q.krow + (size_t)sp * M * Wd, sizeof(double) * M * Wd, hipMemcpyHostToDevice, c->stream));
    ZIGP_TRY(stage_upload_rows(c, white ? lt.a1gm : lt.du, q.du, M, Mp, 1));
    ZIGP_TRY(stage_upload_rows(c, lt.ell, q.ell, D, std::max(D, MAXD), 1));
    if (lq) ZIGP_TRY(stage_upload_square(c, lt.dLq, q.dLq, M, Mp, 0.0));
    else { ZIGP_TRY(stage_upload_rows(c, lt.dsq, q.dsq, M, Mp, 1)); ZIGP_TRY(stage_upload_rows(c, lt.s, q.s, M, Mp, 1)); }
    if (lq) {     // k_dense_pack loads s[m] and dsq[m] before it looks at q_full and discards what it forms from them: zeros
      ZIGP_TRY(stage_upload_rows(c, lt.dsq, nullptr, 0, Mp, 1));
      ZIGP_TRY(stage_upload_rows(c, lt.s, nullptr, 0, Mp, 1));
    }
  }
  zigp_params pp;
  memset(&pp, 0, sizeof(pp));
  DenseCall k;
  memset(static_cast<void*>(&k.hl), 0, sizeof(k.hl));
  k.p = &pp; k.dX = nullptr; k.dY = nullptr; k.Nrows = 0; k.D = D; k.jitter = 0; k.scale = 1; k.g_offset = 0; k.row_begin = 0; k.row_end = 0;
  k.include_kl = a->include_kl ? 1 : 0; k.predict = false; k.d_out9 = nullptr; k.need_grad = grad; k.has_rows = true;
  k.par = par; k.pw_blocks = a->pw_blocks;
  const bool mean_on = c->mean_on;
  c->mean_on = a->mean_on != 0;
  DensePackArgs pa;
  size_t n = 0;
  const int rc = dense_pack(c, k, pa, n);
  c->mean_on = mean_on;
  ZIGP_TRY(rc);
  if (n != need) return fail_arg(c, "zigp_test_dense_pack: the pack laid out another vector than the caller sized");
  ZIGP_TRY(stage_download_rows(c, c->packed.p, a->out, 1, (int64_t)n));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

}  // extern "C"
