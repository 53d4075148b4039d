// Kronecker (space x time) variant of the zero-inflated GP ELBO path: scripts/onoff.py:143-319 (build_prior_kl,
// build_predict, kron_inf, cost), onofftf/main.py:350-387 (GaussKLkron), onofftf/onoffpred.py:127-200 (predict).
//
// The reference forms the dense (M0*M1) x Nb matrix Kmn, the dense Kronecker inverse and two Nb x Nb products of which only
// the diagonal is used (scripts/onoff.py:206-211).  Here everything stays factored (identities checked on the literal oracle in
// tests/test_cpu_oracle.py::test_kronecker_literal_equals_factored_identities).  Per latent, with P_p = K_p^-1, U = reshape(u),
// S2 = reshape(s^2), Alpha = P0 U P1, panels K_p = k_p(Z_p, X_p) [M_p][N], A_p = P_p K_p:
//     mean_n = sum_i K0[i,n] (Alpha K1)[i,n]                      (= Kmn^T alpha, :209)
//     var_n  = v0 v1 - (K0.A0)_n (K1.A1)_n + sum_i A0[i,n]^2 (S2 A1^2)[i,n]      (= Knn - diag(Kmn^T A - A^T S A), :210-211)
//     KL     = 1/2 [ sum U.Alpha - M0 M1 - sum log s^2 + sum_ij diag(P0)_i diag(P1)_j s_ij^2 + M1 logdet K0 + M0 logdet K1 ]
// K_p^-1 comes from the blocked Cholesky + triangular inverse of the dense path (the reference uses an LU inverse,
// tf.matrix_inverse :192; the two agree to O(cond * eps)).  All O(M_p^2 N) / O(M0 M1 N) products and every reduction over N run
// on the fp64 MFMA GEMM core (operands padded to 128); the reverse pass is hand-derived.
#include "zigp_host.h"
#include "zigp_comm.h"
#include "zigp_kronc.h"

using namespace zigp;

namespace zigp {

struct KronFactor {
  int M = 0, Mq = 0, D = 0, col0 = 0;
  int kind = ZIGP_KERN_RBF;                 // zigp_set_kron_kernel: the factor's kernel family
  double var = 1.0;
  std::vector<double> ell;
  DevBuf Z, K, L, W, P, T, dP, G, krow;
  DevBuf Kd;                                // panel [Mq][Nc] of a Matern factor's gradient step: K' = -dk / d(r2 / 2) (k_kron_kbuild_matern)
  DevBuf Kp, Ap, Asq, dA, E, PdA, Bx, Cx;   // panels [Mq][Nc]: K_p, A_p, A_p^2, dA_p, E_p, P_p dA_p, (Alpha K_other), (S2 A_other^2)
};

struct KronLatent {
  KronFactor f[2];
  DevBuf U, S, S2, Al, T0, T1, dAl, dS2, dU;   // [Mq0][Mq1]
  DevBuf part;                                 // column sums [4][Nc]: q0, q1, mean, st
  DevBuf gm, gv, dq0, dq1;                     // [Nc]
  DevBuf planes;                               // split-K partial planes
  DevBuf vec;                                  // diag(P0) [Mq0], diag(P1) [Mq1], scalars[8]
};

struct KronState {
  KronLatent lat[2];
  DevBuf X, Y, acc, out9;
};

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
// Factor panel: K[m][n] = var * exp(-0.5 |(z_m - x_n[col0:col0+D]) / ell|^2), rows m >= M are 0 (kern.K(Z_p, xnew), :199-201)
__global__ void __launch_bounds__(256)
k_kron_kbuild(const double* __restrict__ X, int64_t N, int ldx, int col0, const double* __restrict__ Z, int M, KernHyp h,
              double* __restrict__ K, int64_t Nc) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int m0 = blockIdx.y * 16;
  double xs[MAXD];
  const bool valid = n < N;
#pragma unroll
  for (int d = 0; d < MAXD; ++d) xs[d] = (d < h.D && valid) ? X[n * ldx + col0 + d] * h.inv_ell[d] : 0.0;
#pragma unroll 4
  for (int mm = 0; mm < 16; ++mm) {
    const int m = m0 + mm;
    double v = 0.0;
    if (m < M) {
      double r2 = 0.0;
#pragma unroll
      for (int d = 0; d < MAXD; ++d)
        if (d < h.D) { double t = Z[m * h.D + d] * h.inv_ell[d] - xs[d]; r2 = fma(t, t, r2); }
      const double a = -0.5 * r2;
      v = h.var * exp(a);
      // A subnormal result: exp has already rounded to the subnormal grid and the product with var rounds again (up to 1.4 of the smallest
      // subnormal off).  exp(a / 2) is normal there, so (var e) e rounds once.  Normal results keep the plain product.
      if (v < 0x1p-1021) { const double e = exp(0.5 * a); v = (h.var * e) * e; }
    }
    K[(int64_t)m * Nc + n] = v;
  }
}

__global__ void k_square_panel(const double* __restrict__ A, double* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const double a = A[i]; out[i] = a * a; }
}

// column sums: part[0]=sum_i K0.A0, [1]=sum_j K1.A1, [2]=sum_i K0.B1 (mean), [3]=sum_i A0^2.C1
__global__ void __launch_bounds__(256)
k_kron_colsum(const double* __restrict__ K0, const double* __restrict__ A0, const double* __restrict__ K1, const double* __restrict__ A1,
              const double* __restrict__ B1, const double* __restrict__ A0sq, const double* __restrict__ C1, int M0, int M1, int64_t Nc,
              double* __restrict__ part) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double q0 = 0, q1 = 0, mu = 0, st = 0;
  for (int i = 0; i < M0; ++i) {
    const int64_t o = (int64_t)i * Nc + n;
    q0 = fma(K0[o], A0[o], q0);
    mu = fma(K0[o], B1[o], mu);
    st = fma(A0sq[o], C1[o], st);
  }
  for (int j = 0; j < M1; ++j) {
    const int64_t o = (int64_t)j * Nc + n;
    q1 = fma(K1[o], A1[o], q1);
  }
  part[0 * Nc + n] = q0; part[1 * Nc + n] = q1; part[2 * Nc + n] = mu; part[3 * Nc + n] = st;
}

constexpr int KPW_ACC = 5;
struct KronPwArgs {
  const double* part_f; const double* part_g; const double* Y; int64_t N, Nc;
  double knn_f, knn_g, noise, g_offset, f_offset, scale;   // f_offset: the constant f_mu added to fmean (scripts/onoff.py:168-169, classifier.py:136-137)
  double *gm_f, *gv_f, *gm_g, *gv_g, *dq0_f, *dq1_f, *dq0_g, *dq1_g;
  double* acc;   // [blocks][KPW_ACC]: var_exp, d noise, sum gv_f, sum gv_g, sum gm_f (= d / d f_mu)
  double* out9; int64_t ld9;
  const double* hyp;   // nullable: device hyperparameter block (KH_*): knn_f, knn_g, noise are read from it instead of the fields above
};

template <bool PREDICT>
__global__ void __launch_bounds__(PW_THREADS)
k_kron_pointwise(KronPwArgs p) {
  __shared__ double sh[4];
  const int64_t n = (int64_t)blockIdx.x * PW_THREADS + threadIdx.x;
  // Knn = var_0 var_1 (scripts/onoff.py:196-200): the product of the two factor variances of the latent's records
  const double knn_f = p.hyp ? KF_CONST(p.hyp)[KH_VAR] * KF_CONST(p.hyp)[KH_FAC + KH_VAR] : p.knn_f;
  const double knn_g = p.hyp ? KF_CONST(p.hyp)[2 * KH_FAC + KH_VAR] * KF_CONST(p.hyp)[3 * KH_FAC + KH_VAR] : p.knn_g;
  const double noise = p.hyp ? KF_CONST(p.hyp)[KH_NOISE] : p.noise;
  const double q0f = p.part_f[n], q1f = p.part_f[p.Nc + n], q0g = p.part_g[n], q1g = p.part_g[p.Nc + n];
  const double fm = p.part_f[2 * p.Nc + n] + p.f_offset, fv = knn_f - q0f * q1f + p.part_f[3 * p.Nc + n];
  const double gmn = p.part_g[2 * p.Nc + n] + p.g_offset, gvr = knn_g - q0g * q1g + p.part_g[3 * p.Nc + n];
  const bool valid = n < p.N;
  const double y = (valid && p.Y) ? p.Y[n] : 0.0;
  PwOut o = pointwise_eval(fm, fv, gmn, gvr, y, noise);
  if (PREDICT) {
    if (valid) {
      double* q = p.out9 + n;
      q[0 * p.ld9] = o.gfmean; q[1 * p.ld9] = o.gfvar; q[2 * p.ld9] = o.gfmeanu; q[3 * p.ld9] = fm; q[4 * p.ld9] = fv;
      q[5 * p.ld9] = gmn; q[6 * p.ld9] = gvr; q[7 * p.ld9] = o.e1; q[8 * p.ld9] = o.ev;
    }
    return;
  }
  const double sc = valid ? p.scale : 0.0;
  if (p.gm_f) {
    const double gvf = sc * o.dfv, gvg = sc * o.dgv;
    p.gm_f[n] = sc * o.dfm; p.gv_f[n] = gvf; p.gm_g[n] = sc * o.dgm; p.gv_g[n] = gvg;
    p.dq0_f[n] = -gvf * q1f; p.dq1_f[n] = -gvf * q0f; p.dq0_g[n] = -gvg * q1g; p.dq1_g[n] = -gvg * q0g;
  }
  double s0 = block_sum<4>(valid ? p.scale * o.ve : 0.0, sh);
  double s1 = block_sum<4>(sc * o.dnoise, sh);
  double s2 = block_sum<4>(sc * o.dfv, sh);
  double s3 = block_sum<4>(sc * o.dgv, sh);
  double s4 = block_sum<4>(sc * o.dfm, sh);
  if (threadIdx.x == 0) { double* a = p.acc + (int64_t)blockIdx.x * KPW_ACC; a[0] = s0; a[1] = s1; a[2] = s2; a[3] = s3; a[4] = s4; }
}

// Single-latent heads on the same kron_inf (the reference's baselines):
//   lik 1, Gaussian  (scripts/svgp.py:198-200, hurdle.py:217-219):  ve = -1/2 log 2pi - 1/2 log s2 - 1/2 ((y - fm)^2 + fv) / s2
//   lik 2, Bernoulli (scripts/classifier.py:139-140,210-217):       p = probit(fm / sqrt(1 + fv)),  ve = log(y == 1 ? p : 1 - p)
// with fm = kron mean + f_mu (classifier.py:136-137).  acc[b] = {ve, d noise, sum gv, 0, sum gm (= d f_mu)}.
// Predict rows (ld = N): fmean, fvar, pfmean, pfvar -- Gaussian: pfmean = fm, pfvar = fv + s2 (density of y);
// Bernoulli: pfmean = p, pfvar = p - p^2 (classifier.py:140).
// DEVHYP (the steps of a fit call, zigp_kron_head_fit_steps): Knn = var_0 var_1, the noise and f_mu come from the device hyperparameter
// block the previous step's update wrote (KH_VAR of the two factor records, KH_NOISE, KH_FMU) instead of the by-value fields.
template <bool PREDICT, bool DEVHYP>
__global__ void __launch_bounds__(PW_THREADS)
k_kron_head_pointwise(KronPwArgs p, int lik) {
  __shared__ double sh[4];
  const int64_t n = (int64_t)blockIdx.x * PW_THREADS + threadIdx.x;
  // Knn as the ROUNDED product the by-value launches are handed, and the variance in one association for every variant: left to the
  // compiler, the device-block variant fused var_0 var_1 into the subtraction and rounded q0 q1 on its own instead, an ulp of q0 q1 away
  // from the other launches (what is left of a small predictive variance after the cancellation then differs in its leading digits).
  const double knn_f = DEVHYP ? __dmul_rn(KF_CONST(p.hyp)[KH_VAR], KF_CONST(p.hyp)[KH_FAC + KH_VAR]) : p.knn_f;
  const double noise = DEVHYP ? KF_CONST(p.hyp)[KH_NOISE] : p.noise;
  const double f_offset = DEVHYP ? KF_CONST(p.hyp)[KH_FMU] : p.f_offset;
  const double q0 = p.part_f[n], q1 = p.part_f[p.Nc + n];
  const double fm = p.part_f[2 * p.Nc + n] + f_offset, fv = fma(-q0, q1, knn_f) + p.part_f[3 * p.Nc + n];
  const bool valid = n < p.N;
  const double y = (valid && p.Y) ? p.Y[n] : 0.0;
  double ve, dfm, dfv, dnoise = 0.0, pm, pv;
  if (lik == ZIGP_LIK_GAUSSIAN) {
    const double inv = 1.0 / noise, res = y - fm, q = res * res + fv;
    ve = -0.5 * 1.8378770664093454836 - 0.5 * log(noise) - 0.5 * q * inv;
    dfm = res * inv; dfv = -0.5 * inv; dnoise = -0.5 * inv + 0.5 * q * inv * inv;
    pm = fm; pv = fv + noise;
  } else {
    const double c1 = 1.0 - 2.e-3, c0 = 1.e-3;
    const double r = 1.0 / sqrt(1.0 + fv), z = fm * r;
    const double pr = 0.5 * (1.0 + erf(z * 0.70710678118654752440)) * c1 + c0;   // classifier.py:216-217
    const bool on = (y == 1.0);                                                  // tf.equal(y, 1) :214
    ve = log(on ? pr : 1.0 - pr);
    const double dp = on ? 1.0 / pr : -1.0 / (1.0 - pr);
    const double dz = dp * c1 * 0.39894228040143267794 * exp(-0.5 * z * z);
    dfm = dz * r; dfv = dz * (-0.5 * z / (1.0 + fv));
    pm = pr; pv = pr - pr * pr;
  }
  if (PREDICT) {
    if (valid) { double* q = p.out9 + n; q[0] = fm; q[p.ld9] = fv; q[2 * p.ld9] = pm; q[3 * p.ld9] = pv; }
    return;
  }
  const double sc = valid ? p.scale : 0.0;
  if (p.gm_f) {
    const double gvf = sc * dfv;
    p.gm_f[n] = sc * dfm; p.gv_f[n] = gvf; p.dq0_f[n] = -gvf * q1; p.dq1_f[n] = -gvf * q0;
  }
  double s0 = block_sum<4>(sc * ve, sh);
  double s1 = block_sum<4>(sc * dnoise, sh);
  double s2 = block_sum<4>(sc * dfv, sh);
  double s4 = block_sum<4>(sc * dfm, sh);
  if (threadIdx.x == 0) { double* a = p.acc + (int64_t)blockIdx.x * KPW_ACC; a[0] = s0; a[1] = s1; a[2] = s2; a[3] = 0.0; a[4] = s4; }
}

// dA[i][n] = 2 A[i][n] gv[n] C[i][n] ; E[i][n] = dq[n] K[i][n] + dA[i][n]
__global__ void k_kron_da(const double* __restrict__ A, const double* __restrict__ C, const double* __restrict__ K,
                          const double* __restrict__ gv, const double* __restrict__ dq, int64_t Nc, int64_t total,
                          double* __restrict__ dA, double* __restrict__ E) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t n = i % Nc;
  const double d = 2.0 * A[i] * gv[n] * C[i];
  dA[i] = d;
  E[i] = fma(dq[n], K[i], d);
}

// factor-kernel cotangent reductions, block per row m:  dK[m,n] = gm[n] B[m,n] + 2 dq[n] A[m,n] + PdA[m,n]
//   krow[m][0] += sum dK K ; krow[m][1+d] += sum dK K (x_d - z_md) ; krow[m][1+D+d] += sum dK K (x_d - z_md)^2
__global__ void __launch_bounds__(256)
k_kron_kgrad(const double* __restrict__ B, const double* __restrict__ A, const double* __restrict__ PdA, const double* __restrict__ K,
             const double* __restrict__ gm, const double* __restrict__ dq, const double* __restrict__ X, int64_t N, int ldx, int col0,
             const double* __restrict__ Z, int M, int D, int64_t Nc, double* __restrict__ krow) {
  __shared__ double sh[4];
  const int m = blockIdx.x;
  if (m >= M) return;
  double zz[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) zz[d] = (d < D) ? Z[m * D + d] : 0.0;
  double s0 = 0.0, s1[MAXD], s2[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) { s1[d] = 0.0; s2[d] = 0.0; }
  const int64_t r = (int64_t)m * Nc;
  for (int64_t n = threadIdx.x; n < N; n += 256) {
    const double dk = fma(gm[n], B[r + n], fma(2.0 * dq[n], A[r + n], PdA[r + n]));
    const double t = dk * K[r + n];
    s0 += t;
#pragma unroll
    for (int d = 0; d < MAXD; ++d)
      if (d < D) {
        const double df = X[n * ldx + col0 + d] - zz[d];
        const double td = t * df;
        s1[d] += td;
        s2[d] = fma(td, df, s2[d]);
      }
  }
  const int W = 2 + 2 * D;
  s0 = block_sum<4>(s0, sh);
  if (threadIdx.x == 0) krow[(int64_t)m * W] += s0;
  for (int d = 0; d < D; ++d) {
    double a = block_sum<4>(s1[d], sh);
    double b = block_sum<4>(s2[d], sh);
    if (threadIdx.x == 0) { krow[(int64_t)m * W + 1 + d] += a; krow[(int64_t)m * W + 1 + D + d] += b; }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Matern 3/2 and 5/2 FACTORS (zigp_set_kron_kernel): each of the four factors (latent f / g x factor 0 / 1) has its own kind.  These
// kernels stand beside the RBF ones above, which keep their arguments and their machine code; a call whose factors are all RBF
// launches none of them.  Formulas, the floored distance and K' = -dk / d(r2 / 2): the Matern block of zigp_kernels.h.
// ------------------------------------------------------------------------------------------------------------------
// One element from its r2, in the plain library arithmetic of matern_k / matern_kd (same expressions; sqrt and exp are shared between
// K and K').  r2 is clamped to 2^996 so that a far pair gives t finite, exp(-t) = +0 and K = K' = finite * 0 = +0, never inf * 0.
// The dense panel's kuf_sqrt + table exponential (kuf_matern) is NOT used: its operand is the sum w = -(16 / ln 2) r2 of inputs
// pre-scaled by KUF_C / ell on the host (Zs, hyp_scale), and its table carries var; this panel forms r2 from z / ell - x / ell as
// k_kron_kbuild does, which is also the definition the path kernel (zigp_kronpaths.hip) shares.  The panel path is bound by its
// GEMMs, not by this kernel.
template <int KIND, bool GRAD>
__device__ __forceinline__ void kron_matern_elem(double var, double r2, double& k, double& kd) {
  static_assert(KIND == KERN_M32 || KIND == KERN_M52, "Matern 3/2 or 5/2");
  const double r = sqrt(fmin(r2, 0x1p+996) + MATERN_FLOOR);
  if (KIND == KERN_M32) {
    const double t = MATERN_SQRT3 * r, e = exp(-t);
    k = var * (1.0 + t) * e;
    if (GRAD) kd = 3.0 * var * e;
  } else {
    const double t = MATERN_SQRT5 * r, e = exp(-t);
    k = var * (1.0 + t + (5.0 / 3.0) * (r * r)) * e;
    if (GRAD) kd = (5.0 / 3.0) * var * (1.0 + t) * e;
  }
}

// k_kron_kbuild for a Matern factor: same grid and thread mapping (256 columns x 16 rows a block), rows m >= M zero, columns n >= N the
// kernel at x = 0; GRAD (a gradient step) also writes the derivative panel K' in the same launch.
template <int KIND, bool GRAD>
__global__ void __launch_bounds__(256)
k_kron_kbuild_matern(const double* __restrict__ X, int64_t N, int ldx, int col0, const double* __restrict__ Z, int M, KernHyp h,
                     double* __restrict__ K, double* __restrict__ Kd, int64_t Nc) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int m0 = blockIdx.y * 16;
  double xs[MAXD];
  const bool valid = n < N;
#pragma unroll
  for (int d = 0; d < MAXD; ++d) xs[d] = (d < h.D && valid) ? X[n * ldx + col0 + d] * h.inv_ell[d] : 0.0;
#pragma unroll 4
  for (int mm = 0; mm < 16; ++mm) {
    const int m = m0 + mm;
    double v = 0.0, vd = 0.0;
    if (m < M) {
      double r2 = 0.0;
#pragma unroll
      for (int d = 0; d < MAXD; ++d)
        if (d < h.D) { double t = Z[m * h.D + d] * h.inv_ell[d] - xs[d]; r2 = fma(t, t, r2); }
      kron_matern_elem<KIND, GRAD>(h.var, r2, v, vd);
    }
    K[(int64_t)m * Nc + n] = v;
    if (GRAD) Kd[(int64_t)m * Nc + n] = vd;
  }
}

// k_kron_kgrad for a Matern factor: the same block-per-row mapping and fixed-order reduction; column 0 takes dK K, the 2 D moment
// columns dK K' with K' read from the derivative panel of the build launch.
__global__ void __launch_bounds__(256)
k_kron_kgrad_matern(const double* __restrict__ B, const double* __restrict__ A, const double* __restrict__ PdA, const double* __restrict__ K,
                    const double* __restrict__ Kd, const double* __restrict__ gm, const double* __restrict__ dq, const double* __restrict__ X,
                    int64_t N, int ldx, int col0, const double* __restrict__ Z, int M, int D, int64_t Nc, double* __restrict__ krow) {
  __shared__ double sh[4];
  const int m = blockIdx.x;
  if (m >= M) return;
  double zz[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) zz[d] = (d < D) ? Z[m * D + d] : 0.0;
  double s0 = 0.0, s1[MAXD], s2[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) { s1[d] = 0.0; s2[d] = 0.0; }
  const int64_t r = (int64_t)m * Nc;
  for (int64_t n = threadIdx.x; n < N; n += 256) {
    const double dk = fma(gm[n], B[r + n], fma(2.0 * dq[n], A[r + n], PdA[r + n]));
    const double t = dk * Kd[r + n];
    s0 = fma(dk, K[r + n], s0);
#pragma unroll
    for (int d = 0; d < MAXD; ++d)
      if (d < D) {
        const double df = X[n * ldx + col0 + d] - zz[d];
        const double td = t * df;
        s1[d] += td;
        s2[d] = fma(td, df, s2[d]);
      }
  }
  const int W = 2 + 2 * D;
  s0 = block_sum<4>(s0, sh);
  if (threadIdx.x == 0) krow[(int64_t)m * W] += s0;
  for (int d = 0; d < D; ++d) {
    double a = block_sum<4>(s1[d], sh);
    double b = block_sum<4>(s2[d], sh);
    if (threadIdx.x == 0) { krow[(int64_t)m * W + 1 + d] += a; krow[(int64_t)m * W + 1 + D + d] += b; }
  }
}

// K_p (Mq, Mq) of a Matern factor: the padded, jittered sibling of k_rbf_matrix with X1 = X2 = Z -- identity in the padding, the
// formula at r = 1e-6 (r2 = 0 through the floored distance) plus jitter on the diagonal.
__global__ void k_kron_matern_matrix(const double* __restrict__ Z, int64_t M, KernHyp h, int kind, double jitter, double* __restrict__ out,
                                     int64_t Mq) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Mq * Mq) return;
  const int64_t i = idx / Mq, j = idx - i * Mq;
  double v;
  if (i < M && j < M) {
    double r2 = 0.0;
    for (int d = 0; d < h.D; ++d) {
      const double t = (Z[i * h.D + d] - Z[j * h.D + d]) * h.inv_ell[d];
      r2 = fma(t, t, r2);
    }
    v = matern_k(kind, h.var, r2) + ((i == j) ? jitter : 0.0);
  } else {
    v = (i == j) ? 1.0 : 0.0;
  }
  out[idx] = v;
}

// out[idx] = sum_s planes[s][idx]
__global__ void k_sum_planes(const double* __restrict__ planes, int S, int64_t n, double* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int s = 0; s < S; ++s) a += planes[(int64_t)s * n + i];
  out[i] = a;
}
// d[i] = A[i][i]
__global__ void k_diag(const double* __restrict__ A, int64_t ld, int n, double* __restrict__ d) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = A[(int64_t)i * ld + i];
}
// KL scalars (one block): out[0] = sum U.Al ; out[1] = sum log s^2 ; out[2] = sum d0_i d1_j s2_ij ; out[3] = ld0 ; out[4] = ld1
__global__ void __launch_bounds__(256)
k_kron_kl(const double* __restrict__ U, const double* __restrict__ Al, const double* __restrict__ S, const double* __restrict__ d0,
          const double* __restrict__ d1, const double* __restrict__ L0, const double* __restrict__ L1, int M0, int M1, int Mq0, int Mq1,
          double* __restrict__ out) {
  __shared__ double sh[4];
  double a = 0, b = 0, c = 0, e = 0, f = 0;
  for (int idx = threadIdx.x; idx < M0 * M1; idx += 256) {
    const int i = idx / M1, j = idx - i * M1;
    const int64_t o = (int64_t)i * Mq1 + j;
    const double s = S[o];
    a = fma(U[o], Al[o], a);
    b += log(s * s);
    c = fma(d0[i] * d1[j], s * s, c);
  }
  for (int i = threadIdx.x; i < M0; i += 256) { const double l = L0[(int64_t)i * Mq0 + i]; e += log(l * l); }
  for (int j = threadIdx.x; j < M1; j += 256) { const double l = L1[(int64_t)j * Mq1 + j]; f += log(l * l); }
  a = block_sum<4>(a, sh); b = block_sum<4>(b, sh); c = block_sum<4>(c, sh); e = block_sum<4>(e, sh); f = block_sum<4>(f, sh);
  if (threadIdx.x == 0) { out[0] = a; out[1] = b; out[2] = c; out[3] = e; out[4] = f; }
}
// dP (in place) = sym(dP_data) - kl * ( 0.5 * Q + diag(0.5 * w) ),  w_i = sum_j dother_j s2[i,j] (p = 0) or sum_i dother_i s2[i,j] (p = 1)
__global__ void k_kron_dp_combine(double* __restrict__ dP, const double* __restrict__ Q, const double* __restrict__ s2,
                                  const double* __restrict__ dother, int p, int Mq, int Mqo, int Mo, int64_t lds2, int with_kl) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Mq * Mq) return;
  const int i = (int)(idx / Mq), j = (int)(idx - (int64_t)i * Mq);
  if (j > i) return;   // handle the pair (i,j),(j,i) once
  double v = 0.5 * (dP[(int64_t)i * Mq + j] + dP[(int64_t)j * Mq + i]);
  if (with_kl) {
    v -= 0.25 * (Q[(int64_t)i * Mq + j] + Q[(int64_t)j * Mq + i]);
    if (i == j) {
      double w = 0.0;
      for (int o = 0; o < Mo; ++o) w = fma(dother[o], (p == 0) ? s2[(int64_t)i * lds2 + o] : s2[(int64_t)o * lds2 + i], w);
      v -= 0.5 * w;
    }
  }
  dP[(int64_t)i * Mq + j] = v; dP[(int64_t)j * Mq + i] = v;
}
// G = -(P dP P) - kl * 0.5 * Mother * P      (T holds P dP P)
__global__ void k_kron_dk(const double* __restrict__ T, const double* __restrict__ P, double coef, int64_t n, double* __restrict__ G) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) G[i] = -T[i] - coef * P[i];
}
// u / s gradients:  gu = dU_data - kl*Al ;  gs = 2 s dS2 - kl*(-1/s + d0_i d1_j s)
__global__ void k_kron_us(const double* __restrict__ dUd, const double* __restrict__ Al, const double* __restrict__ dS2,
                          const double* __restrict__ S, const double* __restrict__ d0, const double* __restrict__ d1, int M0, int M1,
                          int Mq1, int with_kl, double* __restrict__ gu, double* __restrict__ gs) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M0 * M1) return;
  const int i = idx / M1, j = idx - i * M1;
  const int64_t o = (int64_t)i * Mq1 + j;
  const double s = S[o];
  double a = dUd[o], b = 2.0 * s * dS2[o];
  if (with_kl) { a -= Al[o]; b -= (-1.0 / s + d0[i] * d1[j] * s); }
  gu[idx] = a; gs[idx] = b;
}

}  // namespace zigp

namespace {

// C[ra x ca blocks] = op(A) op(B) over nkb k-blocks, full tiles
template <int AL, int BL>
int mm(zigp_ctx* c, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int nbi, int nbj, int nkb) {
  TileList tl;
  ZIGP_TRY(tiles_full(c, nbi, nbj, nkb * (BM / BK), tl));
  return run_gemm<AL, BL, false>(c, tl, mk_args(A, lda, B, ldb, C, ldc), EpiStore());
}

// Test hook of a panel step (zigp_test_kron_panel_step, include/zigp_diag.h).  Each tap is a device-to-device copy enqueued on the
// current stream (the latent's own) right behind the launch that produces the value, into a buffer of its own; flush() downloads them
// once the step has finished.  Host code only: an ordinary call passes no tap and enqueues exactly what it did before.
struct KpTap {
  const zigp_stage_kron_panels* s;
  struct Snap { double* host; DevBuf dev; size_t n; };
  std::vector<Snap> snaps;
  DevBuf inject[2];       // device copies of the injected cotangents [4][N], uploaded before the step
  int64_t facts[ZIGP_KPF_COUNT];
  int snap(zigp_ctx* c, double* host, const double* dev, size_t n) {
    if (!host || n == 0) return 0;
    snaps.emplace_back();
    Snap& q = snaps.back();
    q.host = host; q.n = n;
    ZIGP_ENSURE(c, q.dev, n);
    ZIGP_HIP(c, hipMemcpyAsync(q.dev.p, dev, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  int flush(zigp_ctx* c) {      // the streams are idle
    for (Snap& q : snaps) ZIGP_HIP(c, hipMemcpy(q.host, q.dev.p, sizeof(double) * q.n, hipMemcpyDeviceToHost));
    if (s->facts) memcpy(s->facts, facts, sizeof(facts));
    return 0;
  }
};
// the tap set of latent h (nullptr: an ordinary call); KP_SNAP(field, device pointer, count) is a no-op without one
struct KpTapLat {
  KpTap* tap; int h;
  const zigp_kronp_tap_latent* t() const { return tap ? &tap->s->lat[h] : nullptr; }
  int64_t* facts() const { return tap ? tap->facts + ZIGP_KPF_LAT + h * ZIGP_KPF_PER_LAT : nullptr; }
};
#define KP_SNAP(kp, field, dev, n) do { if ((kp).tap) ZIGP_TRY((kp).tap->snap(c, (kp).t()->field, (dev), (n))); } while (0)

// out[Mqa x Mqb] = PA[Mqa][Nc] diag(scale) PB[Mqb][Nc]^T, split-K over S slices + plane sum
// which: the reduction's index in zigp_kronp_tap_latent::planes_of order (the hook's facts and raw planes)
int nred(zigp_ctx* c, KronLatent& lt, const double* PA, const double* PB, const double* scale, int nba, int nbb, int64_t Nc, double* out,
         KpTapLat kp = {nullptr, 0}, int which = 0) {
  const int nk = (int)(Nc / BK);
  int S = std::max(1, std::min(nk, 512 / std::max(1, nba * nbb)));
  TileList tl;
  ZIGP_TRY(get_tiles(c, "kr_n:" + std::to_string(nba) + ":" + std::to_string(nbb) + ":" + std::to_string(nk) + ":" + std::to_string(S),
                     [&](std::vector<GemmTile>& v) {
                       for (int s = 0; s < S; ++s)
                         for (int bi = 0; bi < nba; ++bi)
                           for (int bj = 0; bj < nbb; ++bj)
                             v.push_back(mk_tile(bi, bj, (int)((int64_t)nk * s / S), (int)((int64_t)nk * (s + 1) / S), s));
                     }, tl));
  const int64_t plane = (int64_t)nba * BM * nbb * BN;
  ZIGP_ENSURE(c, lt.planes, (size_t)S * plane);
  GemmArgs g = mk_args(PA, Nc, PB, Nc, lt.planes.p, (int64_t)nbb * BN);
  g.slice_stride = plane; g.kscale = scale;
  if (scale) ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_KCONTIG, true>(c, tl, g, EpiStore())));
  else ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_KCONTIG, false>(c, tl, g, EpiStore())));
  if (kp.tap) {
    kp.facts()[ZIGP_KPF_S_DP0 + which] = S;
    if (kp.t()->planes_of == which) KP_SNAP(kp, planes, lt.planes.p, (size_t)S * plane);
  }
  hipLaunchKernelGGL(k_sum_planes, dim3(ceil_div(plane, 256)), dim3(256), 0, c->stream, lt.planes.p, S, plane, out);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

// lik != ZIGP_LIK_ONOFF: single latent, only the f fields (and, for the Gaussian head, noise) are read
int validate_kron(zigp_ctx* c, const zigp_kron_params* p, int lik = ZIGP_LIK_ONOFF) {
  if (!p) return fail_arg(c, "kron params is NULL");
  if (lik != ZIGP_LIK_ONOFF && lik != ZIGP_LIK_GAUSSIAN && lik != ZIGP_LIK_BERNOULLI) return fail_arg(c, "unknown likelihood head");
  const bool two = lik == ZIGP_LIK_ONOFF;
  if (p->M0f <= 0 || p->M1f <= 0 || (two && (p->M0g <= 0 || p->M1g <= 0))) return fail_arg(c, "inducing counts must be positive");
  if (p->D0 <= 0 || p->D1 <= 0 || p->D0 > MAXD || p->D1 > MAXD) return fail_arg(c, "factor dimensions must be in [1, 8]");
  if (!p->Z0f || !p->Z1f || !p->ell0f || !p->ell1f || !p->u_fm || !p->u_fs_sqrt) return fail_arg(c, "NULL pointer in kron params");
  if (two && (!p->Z0g || !p->Z1g || !p->ell0g || !p->ell1g || !p->u_gm || !p->u_gs_sqrt)) return fail_arg(c, "NULL pointer in kron params");
  if (!(p->var0f > 0) || !(p->var1f > 0) || (two && (!(p->var0g > 0) || !(p->var1g > 0)))) return fail_arg(c, "variances must be positive");
  if (lik != ZIGP_LIK_BERNOULLI && !(p->noise > 0)) return fail_arg(c, "variances must be positive");
  return 0;
}

// factor MxM forward: K_p (+jitter), L_p, W_p, P_p = W^T W
// kind: the factor's ZIGP_KERN_* (a Matern K_p: k_kron_matern_matrix in place of k_rbf_matrix; everything behind K_p is the same)
int factor_forward(zigp_ctx* c, KronFactor& f, int M, int D, int col0, const double* Z, const double* ell, double var, double jitter,
                   int kind = ZIGP_KERN_RBF, KpTapLat kp = {nullptr, 0}, int q = 0) {
  f.M = M; f.Mq = (int)round_up(M, BM); f.D = D; f.col0 = col0; f.var = var; f.kind = kind;
  f.ell.assign(ell, ell + D);
  const int Mq = f.Mq, nb = Mq / BM, kb = BM / BK;
  const size_t mm_ = (size_t)Mq * Mq;
  ZIGP_TRY(upload_padded(c, f.Z, Z, (size_t)M * D, (size_t)Mq * D));
  ZIGP_ENSURE(c, f.K, mm_); ZIGP_ENSURE(c, f.L, mm_); ZIGP_ENSURE(c, f.W, mm_); ZIGP_ENSURE(c, f.P, mm_); ZIGP_ENSURE(c, f.T, mm_);
  KernHyp hyp = make_hyp(ell, var, D);
  if (kind != ZIGP_KERN_RBF)
    hipLaunchKernelGGL(k_kron_matern_matrix, dim3(ceil_div((int64_t)mm_, 256)), dim3(256), 0, c->stream, f.Z.p, (int64_t)M, hyp, kind, jitter, f.K.p,
                       (int64_t)Mq);
  else
    hipLaunchKernelGGL(k_rbf_matrix, dim3(ceil_div((int64_t)mm_, 256)), dim3(256), 0, c->stream, f.Z.p, (int64_t)M, f.Z.p, (int64_t)M, hyp, jitter,
                       f.K.p, (int64_t)Mq, (int64_t)Mq, (int64_t)Mq);
  ZIGP_HIP(c, hipGetLastError());
  KP_SNAP(kp, f[q].K, f.K.p, mm_);
  ZIGP_HIP(c, hipMemcpyAsync(f.L.p, f.K.p, sizeof(double) * mm_, hipMemcpyDeviceToDevice, c->stream));
  ZIGP_TRY(potrf_trtri(c, f.L.p, f.W.p, f.T.p, Mq, true, M, pivot_tol(var, jitter, c->pivot_rtol)));
  KP_SNAP(kp, f[q].L, f.L.p, mm_);
  KP_SNAP(kp, f[q].W, f.W.p, mm_);
  TileList t;
  ZIGP_TRY(get_tiles(c, "bw_s:" + std::to_string(nb), [&](std::vector<GemmTile>& v) {
    for (int bi = 0; bi < nb; ++bi)
      for (int bj = 0; bj < nb; ++bj) v.push_back(mk_tile(bi, bj, std::max(bi, bj) * kb, nb * kb));
  }, t));
  ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false>(c, t, mk_args(f.W.p, Mq, f.W.p, Mq, f.P.p, Mq), EpiStore())));
  KP_SNAP(kp, f[q].P, f.P.p, mm_);
  return 0;
}

int upload_grid(zigp_ctx* c, DevBuf& b, const double* src, int M0, int M1, int Mq0, int Mq1, bool square) {
  const size_t n = (size_t)Mq0 * Mq1;
  ZIGP_PINNED(c, h, n);   // padded image staged in page-locked memory: the copy is asynchronous
  memset(h, 0, sizeof(double) * n);
  for (int i = 0; i < M0; ++i)
    for (int j = 0; j < M1; ++j) { const double v = src[(size_t)i * M1 + j]; h[(size_t)i * Mq1 + j] = square ? v * v : v; }
  ZIGP_ENSURE(c, b, n);
  ZIGP_HIP(c, hipMemcpyAsync(b.p, h, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  return 0;
}

int latent_setup(zigp_ctx* c, KronLatent& lt, const KronHostLatent& h, int D0, int D1, double jitter, KpTapLat kp = {nullptr, 0}) {
  ZIGP_TRY(factor_forward(c, lt.f[0], h.M[0], D0, 0, h.Z[0], h.ell[0], h.var[0], jitter, h.kind[0], kp, 0));
  ZIGP_TRY(factor_forward(c, lt.f[1], h.M[1], D1, D0, h.Z[1], h.ell[1], h.var[1], jitter, h.kind[1], kp, 1));
  const int M0 = h.M[0], M1 = h.M[1], Mq0 = lt.f[0].Mq, Mq1 = lt.f[1].Mq, nb0 = Mq0 / BM, nb1 = Mq1 / BM;
  ZIGP_TRY(upload_grid(c, lt.U, h.u, M0, M1, Mq0, Mq1, false));
  ZIGP_TRY(upload_grid(c, lt.S, h.s, M0, M1, Mq0, Mq1, false));
  ZIGP_TRY(upload_grid(c, lt.S2, h.s, M0, M1, Mq0, Mq1, true));
  const size_t g = (size_t)Mq0 * Mq1;
  ZIGP_ENSURE(c, lt.Al, g); ZIGP_ENSURE(c, lt.T0, g); ZIGP_ENSURE(c, lt.T1, g);
  // Alpha = P0 (U P1) : T0 = U P1 ; Al = P0 T0
  ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.U.p, Mq1, lt.f[1].P.p, Mq1, lt.T0.p, Mq1, nb0, nb1, nb1)));
  ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.f[0].P.p, Mq0, lt.T0.p, Mq1, lt.Al.p, Mq1, nb0, nb1, nb0)));
  ZIGP_ENSURE(c, lt.vec, (size_t)Mq0 + Mq1 + 8);
  hipLaunchKernelGGL(k_diag, dim3(ceil_div(Mq0, 256)), dim3(256), 0, c->stream, lt.f[0].P.p, (int64_t)Mq0, Mq0, lt.vec.p);
  hipLaunchKernelGGL(k_diag, dim3(ceil_div(Mq1, 256)), dim3(256), 0, c->stream, lt.f[1].P.p, (int64_t)Mq1, Mq1, lt.vec.p + Mq0);
  ZIGP_HIP(c, hipGetLastError());
  if (kp.tap) {
    int64_t* fa = kp.facts();
    fa[ZIGP_KPF_MQ0] = Mq0; fa[ZIGP_KPF_MQ1] = Mq1; fa[ZIGP_KPF_NB0] = nb0; fa[ZIGP_KPF_NB1] = nb1;
    KP_SNAP(kp, U, lt.U.p, g); KP_SNAP(kp, S2, lt.S2.p, g); KP_SNAP(kp, T0, lt.T0.p, g); KP_SNAP(kp, Al, lt.Al.p, g);
    KP_SNAP(kp, vec, lt.vec.p, (size_t)Mq0 + Mq1);
  }
  return 0;
}

// K_p panel of a Matern factor (and, with_kd, its derivative panel K' for the gradient step) on k_kron_kbuild's grid
int factor_kbuild_matern(zigp_ctx* c, KronFactor& f, const double* dX, int64_t N, int64_t Nc, int ldx, bool with_kd) {
  const KernHyp hyp = make_hyp(f.ell.data(), f.var, f.D);
  const dim3 grid((unsigned)(Nc / 256), f.Mq / 16), block(256);
  if (with_kd) ZIGP_ENSURE(c, f.Kd, (size_t)f.Mq * Nc);
#define ZIGP_KRON_KB(KK, GG) \
  hipLaunchKernelGGL((k_kron_kbuild_matern<KK, GG>), grid, block, 0, c->stream, dX, N, ldx, f.col0, f.Z.p, f.M, hyp, f.Kp.p, GG ? f.Kd.p : nullptr, Nc)
  if (f.kind == ZIGP_KERN_MATERN32) { if (with_kd) ZIGP_KRON_KB(KERN_M32, true); else ZIGP_KRON_KB(KERN_M32, false); }
  else { if (with_kd) ZIGP_KRON_KB(KERN_M52, true); else ZIGP_KRON_KB(KERN_M52, false); }
#undef ZIGP_KRON_KB
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

// forward panels + column sums for one latent; with_kd: a gradient step (a Matern factor also keeps its derivative panel)
int latent_forward_panels(zigp_ctx* c, KronLatent& lt, const double* dX, int64_t N, int64_t Nc, int ldx, bool with_kd = false) {
  const int nbn = (int)(Nc / BN);
  for (int p = 0; p < 2; ++p) {
    KronFactor& f = lt.f[p];
    const size_t pn = (size_t)f.Mq * Nc;
    ZIGP_ENSURE(c, f.Kp, pn); ZIGP_ENSURE(c, f.Ap, pn); ZIGP_ENSURE(c, f.Asq, pn);
    if (f.kind != ZIGP_KERN_RBF) ZIGP_TRY(factor_kbuild_matern(c, f, dX, N, Nc, ldx, with_kd));
    else {
      KernHyp hyp = make_hyp(f.ell.data(), f.var, f.D);
      hipLaunchKernelGGL(k_kron_kbuild, dim3((unsigned)(Nc / 256), f.Mq / 16), dim3(256), 0, c->stream, dX, N, ldx, f.col0, f.Z.p, f.M, hyp,
                         f.Kp.p, Nc);
      ZIGP_HIP(c, hipGetLastError());
    }
    // A_p = P_p K_p
    ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, f.P.p, f.Mq, f.Kp.p, Nc, f.Ap.p, Nc, f.Mq / BM, nbn, f.Mq / BM)));
    hipLaunchKernelGGL(k_square_panel, dim3(ceil_div((int64_t)pn, 256)), dim3(256), 0, c->stream, f.Ap.p, f.Asq.p, (int64_t)pn);
  }
  KronFactor &f0 = lt.f[0], &f1 = lt.f[1];
  ZIGP_ENSURE(c, f0.Bx, (size_t)f0.Mq * Nc); ZIGP_ENSURE(c, f0.Cx, (size_t)f0.Mq * Nc);
  // B1 = Alpha K1 ; C1 = S2 A1^2   (both [Mq0][Nc])
  ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.Al.p, f1.Mq, f1.Kp.p, Nc, f0.Bx.p, Nc, f0.Mq / BM, nbn, f1.Mq / BM)));
  ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.S2.p, f1.Mq, f1.Asq.p, Nc, f0.Cx.p, Nc, f0.Mq / BM, nbn, f1.Mq / BM)));
  ZIGP_ENSURE(c, lt.part, (size_t)4 * Nc);
  hipLaunchKernelGGL(k_kron_colsum, dim3((unsigned)(Nc / 256)), dim3(256), 0, c->stream, f0.Kp.p, f0.Ap.p, f1.Kp.p, f1.Ap.p, f0.Bx.p, f0.Asq.p,
                     f0.Cx.p, f0.M, f1.M, Nc, lt.part.p);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

int latent_backward(zigp_ctx* c, KronLatent& lt, const double* dX, int64_t N, int64_t Nc, int ldx, bool with_kl, KpTapLat kp = {nullptr, 0}) {
  KronFactor &f0 = lt.f[0], &f1 = lt.f[1];
  const int nbn = (int)(Nc / BN), nb0 = f0.Mq / BM, nb1 = f1.Mq / BM;
  const int Mq0 = f0.Mq, Mq1 = f1.Mq;
  // B0 = Alpha^T K0 ; C0 = S2^T A0^2   ([Mq1][Nc])
  ZIGP_ENSURE(c, f1.Bx, (size_t)Mq1 * Nc); ZIGP_ENSURE(c, f1.Cx, (size_t)Mq1 * Nc);
  ZIGP_TRY((mm<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.Al.p, Mq1, f0.Kp.p, Nc, f1.Bx.p, Nc, nb1, nbn, nb0)));
  ZIGP_TRY((mm<LAY_MNCONTIG, LAY_MNCONTIG>(c, lt.S2.p, Mq1, f0.Asq.p, Nc, f1.Cx.p, Nc, nb1, nbn, nb0)));
  double* dq[2] = {lt.dq0.p, lt.dq1.p};
  for (int p = 0; p < 2; ++p) {
    KronFactor& f = lt.f[p];
    const size_t pn = (size_t)f.Mq * Nc;
    ZIGP_ENSURE(c, f.dA, pn); ZIGP_ENSURE(c, f.E, pn); ZIGP_ENSURE(c, f.PdA, pn);
    ZIGP_ENSURE(c, f.krow, (size_t)f.Mq * (2 + 2 * f.D));
    ZIGP_HIP(c, hipMemsetAsync(f.krow.p, 0, sizeof(double) * f.Mq * (2 + 2 * f.D), c->stream));
    hipLaunchKernelGGL(k_kron_da, dim3(ceil_div((int64_t)pn, 256)), dim3(256), 0, c->stream, f.Ap.p, f.Cx.p, f.Kp.p, lt.gv.p, dq[p], Nc,
                       (int64_t)pn, f.dA.p, f.E.p);
    ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, f.P.p, f.Mq, f.dA.p, Nc, f.PdA.p, Nc, f.Mq / BM, nbn, f.Mq / BM)));
    if (f.kind != ZIGP_KERN_RBF)
      hipLaunchKernelGGL(k_kron_kgrad_matern, dim3(f.Mq), dim3(256), 0, c->stream, f.Bx.p, f.Ap.p, f.PdA.p, f.Kp.p, f.Kd.p, lt.gm.p, dq[p], dX, N, ldx,
                         f.col0, f.Z.p, f.M, f.D, Nc, f.krow.p);
    else
      hipLaunchKernelGGL(k_kron_kgrad, dim3(f.Mq), dim3(256), 0, c->stream, f.Bx.p, f.Ap.p, f.PdA.p, f.Kp.p, lt.gm.p, dq[p], dX, N, ldx, f.col0,
                         f.Z.p, f.M, f.D, Nc, f.krow.p);
    ZIGP_HIP(c, hipGetLastError());
    KP_SNAP(kp, f[p].krow_n, f.krow.p, (size_t)f.Mq * (2 + 2 * f.D));
    // dP_p (data) = E_p K_p^T
    ZIGP_ENSURE(c, f.dP, (size_t)f.Mq * f.Mq);
    ZIGP_TRY(nred(c, lt, f.E.p, f.Kp.p, nullptr, f.Mq / BM, f.Mq / BM, Nc, f.dP.p, kp, p));
    KP_SNAP(kp, f[p].dP_red, f.dP.p, (size_t)f.Mq * f.Mq);
  }
  const size_t g = (size_t)Mq0 * Mq1;
  ZIGP_ENSURE(c, lt.dAl, g); ZIGP_ENSURE(c, lt.dS2, g); ZIGP_ENSURE(c, lt.dU, g);
  // dAlpha = K0 diag(gm) K1^T ; dS2 = A0^2 diag(gv) (A1^2)^T
  ZIGP_TRY(nred(c, lt, f0.Kp.p, f1.Kp.p, lt.gm.p, nb0, nb1, Nc, lt.dAl.p, kp, 2));
  KP_SNAP(kp, dAl, lt.dAl.p, g);
  ZIGP_TRY(nred(c, lt, f0.Asq.p, f1.Asq.p, lt.gv.p, nb0, nb1, Nc, lt.dS2.p, kp, 3));
  KP_SNAP(kp, dS2, lt.dS2.p, g);
  // ---- MxM: Alpha = P0 U P1 ----
  // dU = P0 dAl P1 : T1 = dAl P1 ; dU = P0 T1
  ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, lt.dAl.p, Mq1, f1.P.p, Mq1, lt.T1.p, Mq1, nb0, nb1, nb1)));
  KP_SNAP(kp, T1_a, lt.T1.p, g);
  ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, f0.P.p, Mq0, lt.T1.p, Mq1, lt.dU.p, Mq1, nb0, nb1, nb0)));
  KP_SNAP(kp, dU, lt.dU.p, g);
  // dP0 += dAl (U P1)^T = dAl T0^T  (T0 = U P1 from setup) ; dP1 += (P0 U)^T dAl
  {
    TileList t;
    ZIGP_TRY(tiles_full(c, nb0, nb0, nb1 * (BM / BK), t));
    ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_KCONTIG, false>(c, t, mk_args(lt.dAl.p, Mq1, lt.T0.p, Mq1, f0.dP.p, Mq0), EpiAccum())));
    KP_SNAP(kp, f[0].dP_acc, f0.dP.p, (size_t)Mq0 * Mq0);
    // T1 = P0 U  ([Mq0][Mq1]) ; dP1 += T1^T dAl
    ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, f0.P.p, Mq0, lt.U.p, Mq1, lt.T1.p, Mq1, nb0, nb1, nb0)));
    KP_SNAP(kp, T1_b, lt.T1.p, g);
    TileList t2;
    ZIGP_TRY(tiles_full(c, nb1, nb1, nb0 * (BM / BK), t2));
    ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false>(c, t2, mk_args(lt.T1.p, Mq1, lt.dAl.p, Mq1, f1.dP.p, Mq1), EpiAccum())));
    KP_SNAP(kp, f[1].dP_acc, f1.dP.p, (size_t)Mq1 * Mq1);
  }
  // KL pieces on P: Q0 = U P1 U^T = T0 U^T ; Q1 = U^T P0 U = U^T T1(P0 U)
  for (int p = 0; p < 2; ++p) {
    KronFactor& f = lt.f[p];
    const int Mq = f.Mq, nb = Mq / BM;
    ZIGP_ENSURE(c, f.G, (size_t)Mq * Mq);
    if (with_kl) {
      if (p == 0) {
        TileList t; ZIGP_TRY(tiles_full(c, nb0, nb0, nb1 * (BM / BK), t));
        ZIGP_TRY((run_gemm<LAY_KCONTIG, LAY_KCONTIG, false>(c, t, mk_args(lt.T0.p, Mq1, lt.U.p, Mq1, f.G.p, Mq0), EpiStore())));
      } else {
        TileList t; ZIGP_TRY(tiles_full(c, nb1, nb1, nb0 * (BM / BK), t));
        ZIGP_TRY((run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false>(c, t, mk_args(lt.U.p, Mq1, lt.T1.p, Mq1, f.G.p, Mq1), EpiStore())));
      }
      KP_SNAP(kp, f[p].Q, f.G.p, (size_t)Mq * Mq);
    }
    const KronFactor& fo = lt.f[1 - p];
    hipLaunchKernelGGL(k_kron_dp_combine, dim3(ceil_div((int64_t)Mq * Mq, 256)), dim3(256), 0, c->stream, f.dP.p, f.G.p, lt.S2.p,
                       lt.vec.p + (p == 0 ? Mq0 : 0), p, Mq, fo.Mq, fo.M, (int64_t)Mq1, with_kl ? 1 : 0);
    KP_SNAP(kp, f[p].dP_comb, f.dP.p, (size_t)Mq * Mq);
    // G = -(P dP P) - kl * 0.5 * M_other * P :  T = dP P ; Kt = P T
    ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, f.dP.p, Mq, f.P.p, Mq, f.T.p, Mq, nb, nb, nb)));
    KP_SNAP(kp, f[p].T, f.T.p, (size_t)Mq * Mq);
    // P dP P goes into L: the KL scalars (k_kron_kl, which takes the log-determinants from L) are enqueued before the backward pass
    ZIGP_TRY((mm<LAY_KCONTIG, LAY_MNCONTIG>(c, f.P.p, Mq, f.T.p, Mq, f.L.p, Mq, nb, nb, nb)));
    KP_SNAP(kp, f[p].PdPP, f.L.p, (size_t)Mq * Mq);
    ZIGP_HIP(c, hipGetLastError());
  }
  return 0;
}

}  // namespace

#include "zigp_kronf.hip"

// Defined here, where KronState and KfState are complete.  The members go in reverse order of declaration, then the streams and
// events of the base (zigp_ctx.h).
zigp_ctx::~zigp_ctx() = default;

namespace {

int kron_run_panels(zigp_ctx* c, const KronCall& k, KpTap* tap = nullptr);

// Data-parallel exchange of the PANEL path (grids beyond the fused kernels' capacity): its results reach the host piecewise, so with a
// communicator (zigp_comm_init) the assembled outputs take one more round trip -- packed, summed over ranks on the device, unpacked.
// (The fused path reduces its device result block in place before its single download.)
int kron_exchange_host(zigp_ctx* c, const KronCall& k) {
  if (!c->comm) return 0;
  const zigp_kron_params* p = k.p;
  const int nlat = k.nlat;
  double *elbo_data = k.elbo_data, *kl = k.kl, *d_offset = k.d_offset;
  zigp_kron_grads* g = k.need_grad ? k.grads : nullptr;
  struct Piece { double* p; size_t n; };
  std::vector<Piece> pc;
  double scal[11] = {elbo_data ? *elbo_data : 0.0, kl ? *kl : 0.0, d_offset ? *d_offset : 0.0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (g) { scal[3] = g->var0f; scal[4] = g->var1f; scal[5] = g->var0g; scal[6] = g->var1g; scal[7] = g->noise; }
  pc.push_back({scal, 11});
  if (g) {
    const int M0[2] = {p->M0f, p->M0g}, M1[2] = {p->M1f, p->M1g};
    double* Z0[2] = {g->Z0f, g->Z0g}; double* Z1[2] = {g->Z1f, g->Z1g}; double* l0[2] = {g->ell0f, g->ell0g}; double* l1[2] = {g->ell1f, g->ell1g};
    double* um[2] = {g->u_fm, g->u_gm}; double* us[2] = {g->u_fs_sqrt, g->u_gs_sqrt};
    for (int h = 0; h < nlat; ++h) {
      if (Z0[h]) pc.push_back({Z0[h], (size_t)M0[h] * p->D0});
      if (Z1[h]) pc.push_back({Z1[h], (size_t)M1[h] * p->D1});
      if (l0[h]) pc.push_back({l0[h], (size_t)p->D0});
      if (l1[h]) pc.push_back({l1[h], (size_t)p->D1});
      if (um[h]) pc.push_back({um[h], (size_t)M0[h] * M1[h]});
      if (us[h]) pc.push_back({us[h], (size_t)M0[h] * M1[h]});
    }
  }
  size_t n = 0;
  for (auto& q : pc) n += q.n;
  ZIGP_TRY(begin_staged_call(c));
  ZIGP_ENSURE(c, c->packed, n);
  ZIGP_PINNED(c, hin, n);
  size_t o = 0;
  for (auto& q : pc) { memcpy(hin + o, q.p, sizeof(double) * q.n); o += q.n; }
  ZIGP_HIP(c, hipMemcpyAsync(c->packed.p, hin, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  ZIGP_TRY(comm_allreduce(c, c->packed.p, n));
  double* hout = nullptr;
  ZIGP_TRY(download(c, c->packed.p, n, &hout));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  o = 0;
  for (auto& q : pc) { memcpy(q.p, hout + o, sizeof(double) * q.n); o += q.n; }
  if (elbo_data) *elbo_data = scal[0];
  if (kl) *kl = scal[1];
  if (d_offset) *d_offset = scal[2];
  if (g) { g->var0f = scal[3]; g->var1f = scal[4]; g->var0g = scal[5]; g->var1g = scal[6]; g->noise = scal[7]; }
  return 0;
}

// Does a call with these factor kinds run on the fused kernels?  RBF factors: always (given the grid, and zigp_set_kron_panels off);
// a Matern factor: only with zigp_set_kron_matern_fused on (the _kinds kernels of zigp_kronf.hip; off by default)
static bool kron_kinds_fused(const zigp_ctx* c, const KronHostLatent* hl, int nlat) {
  return c->kron_matern_fused || kron_matern_factor(hl, nlat).empty();
}
// small grids go through the fused register-resident kernels (zigp_kronf.hip); larger factors, and (unless zigp_set_kron_matern_fused
// is on) every call with a Matern factor (zigp_set_kron_kernel), through the panel path below
int kron_run(zigp_ctx* c, const KronCall& k) {
  if (!c->kron_panels && kf_eligible(k.p, k.nlat) && kron_kinds_fused(c, k.hl, k.nlat)) return kronf_run(c, k);
  return kron_run_panels(c, k);
}

int kron_run_panels(zigp_ctx* c, const KronCall& k, KpTap* tap) {
  const zigp_kron_params* p = k.p;
  const double *X = k.X, *Y = k.Y;
  const int64_t N = k.N;
  const int nlat = k.nlat, include_kl = k.include_kl;
  const bool predict = k.predict, need_grad = k.need_grad;
  const KronHostLatent* hl = k.hl;
  if (!c->kron) { c->kron.reset(new (std::nothrow) KronState()); if (!c->kron) { c->err = "out of memory"; return ZIGP_EHIP; } }
  KronState& ks = *c->kron;
  ZIGP_TRY(begin_staged_call(c));
  const int D0 = p->D0, D1 = p->D1, ldx = D0 + D1;
  const int64_t Nc = std::max<int64_t>(1024, round_up(N, 1024));
  if (k.dev_xy) {   // rows of the resident data set: device-to-device
    ZIGP_ENSURE(c, ks.X, (size_t)N * ldx); ZIGP_ENSURE(c, ks.Y, (size_t)N);
    ZIGP_HIP(c, hipMemcpyAsync(ks.X.p, X, sizeof(double) * N * ldx, hipMemcpyDeviceToDevice, c->stream));
    if (Y) ZIGP_HIP(c, hipMemcpyAsync(ks.Y.p, Y, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
  } else {
    ZIGP_TRY(upload_padded(c, ks.X, X, (size_t)N * ldx, (size_t)N * ldx));   // the minibatch, staged like the parameters
    if (Y) ZIGP_TRY(upload_padded(c, ks.Y, Y, (size_t)N, (size_t)N));
  }
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  // the two latents are independent launch chains of small kernels: f on the main stream, g on stream2
  ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
  for (int h = 0; h < nlat; ++h) {
    OnStream on(c, h == 0 ? c->stream_main : c->stream2);
    ZIGP_TRY(latent_setup(c, ks.lat[h], hl[h], D0, D1, k.jitter, KpTapLat{tap, h}));
  }
  ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  int* hinfo = nullptr;
  ZIGP_TRY(request_info(c, &hinfo));   // read after the final synchronisation
  // KL scalars (value) -- before the backward pass overwrites nothing it needs
  double* hkl[2] = {nullptr, nullptr};
  if (include_kl && !predict) {
    for (int h = 0; h < nlat; ++h) {
      KronLatent& lt = ks.lat[h];
      const int Mq0 = lt.f[0].Mq, Mq1 = lt.f[1].Mq;
      hipLaunchKernelGGL(k_kron_kl, dim3(1), dim3(256), 0, c->stream, lt.U.p, lt.Al.p, lt.S.p, lt.vec.p, lt.vec.p + Mq0, lt.f[0].L.p, lt.f[1].L.p,
                         lt.f[0].M, lt.f[1].M, Mq0, Mq1, lt.vec.p + Mq0 + Mq1);
      KP_SNAP((KpTapLat{tap, h}), klv, lt.vec.p + Mq0 + Mq1, 5);
      ZIGP_TRY(download(c, lt.vec.p + Mq0 + Mq1, 8, &hkl[h]));
    }
  }
  ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
  for (int h = 0; h < nlat; ++h) {
    OnStream on(c, h == 0 ? c->stream_main : c->stream2);
    KronLatent& lt = ks.lat[h];
    ZIGP_TRY(latent_forward_panels(c, lt, ks.X.p, N, Nc, ldx, need_grad));
    KP_SNAP((KpTapLat{tap, h}), part, lt.part.p, (size_t)4 * Nc);
    ZIGP_ENSURE(c, lt.gm, Nc); ZIGP_ENSURE(c, lt.gv, Nc); ZIGP_ENSURE(c, lt.dq0, Nc); ZIGP_ENSURE(c, lt.dq1, Nc);
  }
  ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  const int blocks = (int)(Nc / PW_THREADS);
  ZIGP_ENSURE(c, ks.acc, (size_t)blocks * KPW_ACC);
  KronPwArgs a;
  const int gl_ = nlat - 1;   // latent whose buffers stand in for g (unused by the single-latent kernels)
  a.part_f = ks.lat[0].part.p; a.part_g = ks.lat[gl_].part.p; a.Y = Y ? ks.Y.p : nullptr; a.N = N; a.Nc = Nc;
  a.knn_f = p->var0f * p->var1f; a.knn_g = p->var0g * p->var1g; a.noise = p->noise; a.g_offset = k.g_offset; a.f_offset = k.f_mu; a.scale = k.scale;
  a.gm_f = need_grad ? ks.lat[0].gm.p : nullptr; a.gv_f = ks.lat[0].gv.p; a.gm_g = ks.lat[gl_].gm.p; a.gv_g = ks.lat[gl_].gv.p;
  a.dq0_f = ks.lat[0].dq0.p; a.dq1_f = ks.lat[0].dq1.p; a.dq0_g = ks.lat[gl_].dq0.p; a.dq1_g = ks.lat[gl_].dq1.p;
  a.acc = ks.acc.p; a.out9 = nullptr; a.ld9 = N; a.hyp = nullptr;
  if (predict) {
    const int rows = nlat == 2 ? 9 : 4;
    ZIGP_ENSURE(c, ks.out9, (size_t)rows * N);
    a.out9 = ks.out9.p;
    if (nlat == 2) hipLaunchKernelGGL(k_kron_pointwise<true>, dim3(blocks), dim3(PW_THREADS), 0, c->stream, a);
    else hipLaunchKernelGGL((k_kron_head_pointwise<true, false>), dim3(blocks), dim3(PW_THREADS), 0, c->stream, a, k.lik);
    ZIGP_HIP(c, hipGetLastError());
    ZIGP_HIP(c, hipMemcpyAsync(k.out, ks.out9.p, sizeof(double) * rows * N, hipMemcpyDeviceToHost, c->stream));
    ZIGP_HIP(c, hipStreamSynchronize(c->stream));
    return info_result(c, hinfo, kron_fac_any);
  }
  if (nlat == 2) hipLaunchKernelGGL(k_kron_pointwise<false>, dim3(blocks), dim3(PW_THREADS), 0, c->stream, a);
  else hipLaunchKernelGGL((k_kron_head_pointwise<false, false>), dim3(blocks), dim3(PW_THREADS), 0, c->stream, a, k.lik);
  ZIGP_HIP(c, hipGetLastError());
  double* hacc = nullptr;
  ZIGP_TRY(download(c, ks.acc.p, (size_t)blocks * KPW_ACC, &hacc));
  if (tap) {   // the hook: injected cotangents over what the point-wise launch wrote (columns < N), then the four vectors as the backward pass reads them
    tap->facts[ZIGP_KPF_NC] = Nc; tap->facts[ZIGP_KPF_NK] = Nc / BK;
    for (int h = 0; h < nlat; ++h) {
      KronLatent& lt = ks.lat[h];
      double* const v[4] = {lt.gm.p, lt.gv.p, lt.dq0.p, lt.dq1.p};
      for (int i = 0; i < 4; ++i) {
        if (tap->inject[h].p)
          ZIGP_HIP(c, hipMemcpyAsync(v[i], tap->inject[h].p + (size_t)i * N, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
        if (tap->s->lat[h].cot) ZIGP_TRY(tap->snap(c, tap->s->lat[h].cot + (size_t)i * Nc, v[i], (size_t)Nc));
      }
    }
  }

  double *hkrow[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *hgu[2] = {nullptr, nullptr}, *hgs[2] = {nullptr, nullptr};
  if (need_grad) {
    ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
    for (int h = 0; h < nlat; ++h) {
      OnStream on(c, h == 0 ? c->stream_main : c->stream2);
      KronLatent& lt = ks.lat[h];
      const KpTapLat kp{tap, h};
      ZIGP_TRY(latent_backward(c, lt, ks.X.p, N, Nc, ldx, include_kl != 0, kp));
      const int M0 = lt.f[0].M, M1 = lt.f[1].M, Mq0 = lt.f[0].Mq, Mq1 = lt.f[1].Mq;
      for (int q = 0; q < 2; ++q) {
        KronFactor& f = lt.f[q];
        const int Mq = f.Mq;
        // G = -(P dP P) - kl*0.5*M_other*P  -> f.G ; then Kuu-style reductions into krow
        hipLaunchKernelGGL(k_kron_dk, dim3(ceil_div((int64_t)Mq * Mq, 256)), dim3(256), 0, c->stream, f.L.p, f.P.p,
                           include_kl ? 0.5 * (double)lt.f[1 - q].M : 0.0, (int64_t)Mq * Mq, f.G.p);
        KP_SNAP(kp, f[q].G, f.G.p, (size_t)Mq * Mq);
        if (f.kind != ZIGP_KERN_RBF)
          hipLaunchKernelGGL(k_kuu_grad_matern, dim3(Mq), dim3(256), 0, c->stream, f.G.p, f.K.p, k.jitter, f.Z.p, f.M,
                             make_hyp(f.ell.data(), f.var, f.D), f.kind, (int64_t)Mq, f.krow.p);
        else
          hipLaunchKernelGGL(k_kuu_grad, dim3(Mq), dim3(256), 0, c->stream, f.G.p, f.K.p, k.jitter, f.Z.p, f.M, f.D, (int64_t)Mq, f.krow.p);
        ZIGP_HIP(c, hipGetLastError());
        KP_SNAP(kp, f[q].krow, f.krow.p, (size_t)Mq * (2 + 2 * f.D));
        ZIGP_TRY(download(c, f.krow.p, (size_t)Mq * (2 + 2 * f.D), &hkrow[h][q]));
      }
      // u, s gradients (reuse T0 / T1 as outputs)
      hipLaunchKernelGGL(k_kron_us, dim3(ceil_div((int64_t)M0 * M1, 256)), dim3(256), 0, c->stream, lt.dU.p, lt.Al.p, lt.dS2.p, lt.S.p, lt.vec.p,
                         lt.vec.p + Mq0, M0, M1, Mq1, include_kl ? 1 : 0, lt.T0.p, lt.T1.p);
      ZIGP_HIP(c, hipGetLastError());
      KP_SNAP(kp, gu, lt.T0.p, (size_t)M0 * M1); KP_SNAP(kp, gs, lt.T1.p, (size_t)M0 * M1);
      ZIGP_TRY(download(c, lt.T0.p, (size_t)M0 * M1, &hgu[h]));
      ZIGP_TRY(download(c, lt.T1.p, (size_t)M0 * M1, &hgs[h]));
    }
    ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  }
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  ZIGP_TRY(info_result(c, hinfo, kron_fac_any));
  double s_ve = 0, s_dn = 0, s_gv[2] = {0, 0}, s_gm = 0;
  for (int b = 0; b < blocks; ++b) {
    const double* r = hacc + (size_t)KPW_ACC * b;
    s_ve += r[0]; s_dn += r[1]; s_gv[0] += r[2]; s_gv[1] += r[3]; s_gm += r[4];
  }
  if (k.elbo_data) *k.elbo_data = s_ve;
  if (k.d_offset) *k.d_offset = s_gm;
  if (k.kl) *k.kl = kron_kl(k, hkl, include_kl ? 1.0 : 0.0);
  if (need_grad) kron_assemble_grads(k, hkrow, hgu, hgs, s_gv, s_dn);
  return kron_exchange_host(c, k);
}

}  // namespace

namespace {
// Prediction sets can be much larger than a training minibatch (predict_onoff runs over the full Xtrain / Xtest): rows go through
// the path in chunks, so device panels and the pinned staging arena stay bounded; the factor stage is recomputed per chunk (microseconds).
constexpr int64_t KRON_PREDICT_CHUNK = 131072;
int kron_predict_chunked(zigp_ctx* c, const KronCall& k) {
  if (k.N <= KRON_PREDICT_CHUNK) return kron_run(c, k);
  const int ldx = k.p->D0 + k.p->D1, rows = k.nlat == 2 ? 9 : 4;
  std::vector<double> tmp((size_t)rows * KRON_PREDICT_CHUNK);
  KronCall kc = k;
  kc.out = tmp.data();
  for (int64_t n0 = 0; n0 < k.N; n0 += KRON_PREDICT_CHUNK) {
    kc.X = k.X + n0 * ldx; kc.N = std::min(KRON_PREDICT_CHUNK, k.N - n0);
    ZIGP_TRY(kron_run(c, kc));
    for (int r = 0; r < rows; ++r) memcpy(k.out + (size_t)r * k.N + n0, tmp.data() + (size_t)r * kc.N, sizeof(double) * kc.N);
  }
  return ZIGP_OK;
}
// An EMPTY row set (a rank of a data-parallel run whose shard is empty) still has to make the same calls as its peers -- the exchange
// inside the step is collective.  It is evaluated as ONE row at the origin with scale 0: the data term and every data-term gradient
// are exactly zero, the KL part follows include_kl as usual.
const double kron_no_rows[2 * MAXD] = {0};

// ---- the entry-point layer: each public function fills a KronCall with its arguments and names itself (`name`, for the messages) and,
// for a single-latent head, its on/off counterpart (`twin`; nullptr for the on/off entry points) ----
int kron_refuse(zigp_ctx* c, const char* name, const std::string& what) { c->err = std::string(name) + ": " + what; return ZIGP_EARG; }

// zigp_kron[_head]_elbo (rows == nullptr: k.N host rows k.X, k.Y) and zigp_kron[_head]_elbo_rows (rows[0] .. rows[1] of the resident data set)
int kron_elbo_entry(zigp_ctx* c, const char* name, const char* twin, KronCall k, const int64_t* rows) {
  if (!c) return ZIGP_EARG;
  if (twin && k.lik == ZIGP_LIK_ONOFF) return kron_refuse(c, name, std::string("use ") + twin + " for the OnOff likelihood");
  ZIGP_TRY(validate_kron(c, k.p, k.lik));
  if (!rows && (k.N < 0 || (k.N > 0 && (!k.X || !k.Y)))) return kron_refuse(c, name, "need X, Y for N > 0 rows");
  if (!(k.jitter >= 0)) return kron_refuse(c, name, "jitter must be >= 0");
  const bool empty = rows ? (rows[0] == rows[1] && rows[0] >= 0 && rows[0] <= c->N) : k.N == 0;
  if (rows && !empty) {
    if (!c->dX) return kron_refuse(c, name, "no data set (call zigp_set_data first)");
    if (k.p->D0 + k.p->D1 != c->D) return kron_refuse(c, name, "D0 + D1 differs from the data's D");
    if (rows[0] < 0 || rows[1] > c->N || rows[0] > rows[1]) return kron_refuse(c, name, "bad row range");
    k.X = c->dX + rows[0] * c->D; k.Y = c->dY + rows[0]; k.N = rows[1] - rows[0]; k.dev_xy = true;
  }
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (empty) { k.X = k.Y = kron_no_rows; k.N = 1; k.scale = 0.0; }      // zero data term, same calls as the peers of an empty shard
  kron_call_derive(k);
  kron_set_kinds(c, k.hl, k.nlat);
  return kron_run(c, k);
}

// zigp_kron[_head]_predict: k.N rows k.X -> k.out
int kron_predict_entry(zigp_ctx* c, const char* name, const char* twin, KronCall k) {
  if (!c) return ZIGP_EARG;
  if (twin && k.lik == ZIGP_LIK_ONOFF) return kron_refuse(c, name, std::string("use ") + twin + " for the OnOff likelihood");
  ZIGP_TRY(validate_kron(c, k.p, k.lik));
  if (k.N < 0 || (k.N > 0 && (!k.X || !k.out))) return kron_refuse(c, name, "bad arguments");
  if (k.N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  k.scale = 1.0; k.predict = true;
  kron_call_derive(k);
  kron_set_kinds(c, k.hl, k.nlat);
  return kron_predict_chunked(c, k);
}

const int32_t* fit_trainable(const zigp_kron_fit_opts*) { return nullptr; }
const int32_t* fit_trainable(const zigp_kron_head_fit_opts* o) { return o->trainable; }

// zigp_kron_fit_steps / zigp_kron_head_fit_steps (Opts tells them apart).  fit: the caller's state, steps and batches; its per-block
// options are taken from opts here, behind the NULL check.  rows_entry: the entry point a grid beyond the fused kernels is sent to.
template <class Opts>
int kron_fit_entry(zigp_ctx* c, const char* name, const char* rows_entry, const Opts* opts, KfFitCall fit, KronCall k) {
  constexpr bool head = std::is_same<Opts, zigp_kron_head_fit_opts>::value;
  const zigp_kron_params* p = k.p;
  if (!c) return ZIGP_EARG;
  c->fit_steps_applied = 0;      // whatever ends this call early, no update of it has been applied
  if (!p || !opts || !fit.x || !fit.m || !fit.v || !fit.row_begin) return kron_refuse(c, name, "NULL argument");
  if (head && k.lik != ZIGP_LIK_GAUSSIAN && k.lik != ZIGP_LIK_BERNOULLI)
    return kron_refuse(c, name, "the likelihood must be ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI (the OnOff fit is zigp_kron_fit_steps)");
  if (p->M0f <= 0 || p->M1f <= 0 || (!head && (p->M0g <= 0 || p->M1g <= 0))) return fail_arg(c, "inducing counts must be positive");
  if (p->D0 <= 0 || p->D1 <= 0 || p->D0 > MAXD || p->D1 > MAXD) return fail_arg(c, "factor dimensions must be in [1, 8]");
  {
    KronHostLatent kinds[2] = {};
    kron_set_kinds(c, kinds, head ? 1 : 2);
    const std::string who = kron_matern_factor(kinds, head ? 1 : 2);
    if (!who.empty() && !c->kron_matern_fused)
      return kron_refuse(c, name, "a " + who + " is set (zigp_set_kron_kernel); the device loop fits RBF factors only: step it with " + rows_entry +
                                      " and a host optimiser");
  }
  if (fit.n_steps <= 0 || fit.batch <= 0 || fit.t0 < 0) return kron_refuse(c, name, "need n_steps > 0, batch > 0, t0 >= 0");
  if (!(k.jitter >= 0)) return kron_refuse(c, name, "jitter must be >= 0");
  if (!(opts->beta1 >= 0 && opts->beta1 < 1 && opts->beta2 >= 0 && opts->beta2 < 1 && opts->eps > 0)) return kron_refuse(c, name, "bad Adam constants");
  if (!c->dX) return kron_refuse(c, name, "no data set (call zigp_set_data first)");
  if (p->D0 + p->D1 != c->D) return kron_refuse(c, name, "D0 + D1 differs from the data's D");
  if (c->kron_panels || !kf_eligible(p, head ? 1 : 2))
    return kron_refuse(c, name, std::string("this inducing grid is beyond the fused Kronecker kernels (<= 32 x <= 32 or <= 16 x <= 112 points): step it with ") +
                                    rows_entry + " and a host optimiser");
  if (head && fit.n_free != (int64_t)p->M0f * p->D0 + (int64_t)p->M1f * p->D1 + 2 * (int64_t)p->M0f * p->M1f + p->D0 + p->D1 + 4)
    return kron_refuse(c, name, "n_free does not match the model sizes");
  for (int i = 0; i < fit.n_steps; ++i) {
    if (fit.row_begin[i] >= 0 ? fit.row_begin[i] + fit.batch > c->N : (!fit.Xw || !fit.Yw))
      return kron_refuse(c, name, "a row range leaves the resident data set (or a host batch without Xw / Yw)");
  }
  ZIGP_HIP(c, hipSetDevice(c->device));
  fit.name = name; fit.head = head;
  fit.lr = opts->lr; fit.positive = opts->positive; fit.trainable = fit_trainable(opts);
  fit.beta1 = opts->beta1; fit.beta2 = opts->beta2; fit.eps = opts->eps;
  k.X = c->dX; k.Y = c->dY; k.N = fit.batch; k.dev_xy = true;      // p carries the sizes only: the parameters come from the free state
  kron_call_derive(k);
  kron_set_kinds(c, k.hl, k.nlat);      // Matern factors get here with zigp_set_kron_matern_fused only (refused above otherwise)
  k.need_grad = true;
  return kronf_run(c, k, &fit);
}
}  // namespace

extern "C" {

int zigp_kron_elbo(zigp_ctx* c, const zigp_kron_params* p, const double* X, const double* Y, int64_t N, double jitter, double scale,
                   double g_offset, double f_mu, int32_t include_kl, double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu) {
  KronCall k = {};
  k.p = p; k.lik = ZIGP_LIK_ONOFF; k.X = X; k.Y = Y; k.N = N; k.jitter = jitter; k.scale = scale; k.g_offset = g_offset; k.f_mu = f_mu;
  k.include_kl = include_kl; k.elbo_data = elbo_data; k.kl = kl; k.grads = grads; k.d_offset = d_f_mu;
  return kron_elbo_entry(c, "zigp_kron_elbo", nullptr, k, nullptr);
}

int zigp_kron_elbo_rows(zigp_ctx* c, const zigp_kron_params* p, int64_t row_begin, int64_t row_end, double jitter, double scale, double g_offset,
                        double f_mu, int32_t include_kl, double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu) {
  const int64_t rows[2] = {row_begin, row_end};
  KronCall k = {};
  k.p = p; k.lik = ZIGP_LIK_ONOFF; k.jitter = jitter; k.scale = scale; k.g_offset = g_offset; k.f_mu = f_mu;
  k.include_kl = include_kl; k.elbo_data = elbo_data; k.kl = kl; k.grads = grads; k.d_offset = d_f_mu;
  return kron_elbo_entry(c, "zigp_kron_elbo_rows", nullptr, k, rows);
}

int zigp_kron_head_elbo(zigp_ctx* c, const zigp_kron_params* p, int32_t lik, const double* X, const double* Y, int64_t N, double jitter,
                        double scale, double f_mu, int32_t include_kl, double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu) {
  KronCall k = {};
  k.p = p; k.lik = lik; k.X = X; k.Y = Y; k.N = N; k.jitter = jitter; k.scale = scale; k.f_mu = f_mu;
  k.include_kl = include_kl; k.elbo_data = elbo_data; k.kl = kl; k.grads = grads; k.d_offset = d_f_mu;
  return kron_elbo_entry(c, "zigp_kron_head_elbo", "zigp_kron_elbo", k, nullptr);
}

int zigp_kron_head_elbo_rows(zigp_ctx* c, const zigp_kron_params* p, int32_t lik, int64_t row_begin, int64_t row_end, double jitter, double scale,
                             double f_mu, int32_t include_kl, double* elbo_data, double* kl, zigp_kron_grads* grads, double* d_f_mu) {
  const int64_t rows[2] = {row_begin, row_end};
  KronCall k = {};
  k.p = p; k.lik = lik; k.jitter = jitter; k.scale = scale; k.f_mu = f_mu;
  k.include_kl = include_kl; k.elbo_data = elbo_data; k.kl = kl; k.grads = grads; k.d_offset = d_f_mu;
  return kron_elbo_entry(c, "zigp_kron_head_elbo_rows", "zigp_kron_elbo_rows", k, rows);
}

int zigp_kron_predict(zigp_ctx* c, const zigp_kron_params* p, const double* Xnew, int64_t N, double jitter, double g_offset, double f_mu, double* out9) {
  KronCall k = {};
  k.p = p; k.lik = ZIGP_LIK_ONOFF; k.X = Xnew; k.N = N; k.jitter = jitter; k.g_offset = g_offset; k.f_mu = f_mu; k.out = out9;
  return kron_predict_entry(c, "zigp_kron_predict", nullptr, k);
}

int zigp_kron_head_predict(zigp_ctx* c, const zigp_kron_params* p, int32_t lik, const double* Xnew, int64_t N, double jitter, double f_mu,
                           double* out4) {
  KronCall k = {};
  k.p = p; k.lik = lik; k.X = Xnew; k.N = N; k.jitter = jitter; k.f_mu = f_mu; k.out = out4;
  return kron_predict_entry(c, "zigp_kron_head_predict", "zigp_kron_predict", k);
}

int zigp_kron_fit_steps(zigp_ctx* c, const zigp_kron_params* p, const zigp_kron_fit_opts* opts, double* free_state, double* adam_m, double* adam_v,
                        int64_t n_free, int64_t t0, int32_t n_steps, const int64_t* row_begin, int64_t batch, const double* Xw, const double* Yw,
                        double jitter, double scale, int32_t include_kl, double* elbo_data, double* kl) {
  KfFitCall fit = {};
  fit.x = free_state; fit.m = adam_m; fit.v = adam_v; fit.n_free = n_free; fit.t0 = t0; fit.n_steps = (int)n_steps; fit.row_begin = row_begin;
  fit.batch = batch; fit.Xw = Xw; fit.Yw = Yw; fit.hist_data = elbo_data; fit.hist_kl = kl;
  KronCall k = {};
  k.p = p; k.lik = ZIGP_LIK_ONOFF; k.jitter = jitter; k.scale = scale; k.include_kl = include_kl;
  return kron_fit_entry(c, "zigp_kron_fit_steps", "zigp_kron_elbo_rows", opts, fit, k);
}

int zigp_kron_head_fit_steps(zigp_ctx* c, const zigp_kron_params* p, int32_t lik, const zigp_kron_head_fit_opts* opts, double* free_state,
                             double* adam_m, double* adam_v, int64_t n_free, int64_t t0, int32_t n_steps, const int64_t* row_begin, int64_t batch,
                             const double* Xw, const double* Yw, double jitter, double scale, int32_t include_kl, double* elbo_data, double* kl) {
  KfFitCall fit = {};
  fit.x = free_state; fit.m = adam_m; fit.v = adam_v; fit.n_free = n_free; fit.t0 = t0; fit.n_steps = (int)n_steps; fit.row_begin = row_begin;
  fit.batch = batch; fit.Xw = Xw; fit.Yw = Yw; fit.hist_data = elbo_data; fit.hist_kl = kl;
  KronCall k = {};
  k.p = p; k.lik = lik; k.jitter = jitter; k.scale = scale; k.include_kl = include_kl;
  return kron_fit_entry(c, "zigp_kron_head_fit_steps", "zigp_kron_head_elbo_rows", opts, fit, k);
}

int64_t zigp_kron_fit_steps_applied(zigp_ctx* c) { return c ? c->fit_steps_applied : (int64_t)ZIGP_EARG; }


int zigp_set_kron_range_tiles(zigp_ctx* c, int32_t tiles) {
  if (!c) return ZIGP_EARG;
  if (tiles < 1) return fail_arg(c, "zigp_set_kron_range_tiles: need >= 1 tile");
  c->kron_range_tiles = tiles;
  return ZIGP_OK;
}

int zigp_set_kron_kernel(zigp_ctx* c, int32_t latent, int32_t factor, int32_t kind) {
  if (!c) return ZIGP_EARG;
  if (latent != 0 && latent != 1) return fail_arg(c, "zigp_set_kron_kernel: latent must be 0 (f) or 1 (g)");
  if (factor != 0 && factor != 1) return fail_arg(c, "zigp_set_kron_kernel: factor must be 0 or 1");
  if (kind != ZIGP_KERN_RBF && kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52)
    return fail_arg(c, "zigp_set_kron_kernel: unknown kernel kind (ZIGP_KERN_RBF, ZIGP_KERN_MATERN32, ZIGP_KERN_MATERN52)");
  c->kron_kern[latent][factor] = kind;
  return ZIGP_OK;
}

int zigp_get_kron_kernel(zigp_ctx* c, int32_t latent, int32_t factor) {
  if (!c) return ZIGP_EARG;
  if (latent != 0 && latent != 1) return fail_arg(c, "zigp_get_kron_kernel: latent must be 0 (f) or 1 (g)");
  if (factor != 0 && factor != 1) return fail_arg(c, "zigp_get_kron_kernel: factor must be 0 or 1");
  return c->kron_kern[latent][factor];
}

int zigp_set_kron_panels(zigp_ctx* c, int32_t on) {
  if (!c) return ZIGP_EARG;
  c->kron_panels = on != 0;
  return ZIGP_OK;
}

int zigp_set_kron_matern_fused(zigp_ctx* c, int32_t on) {
  if (!c) return ZIGP_EARG;
  if (on != 0 && on != 1) return fail_arg(c, "zigp_set_kron_matern_fused: on must be 0 or 1");
  c->kron_matern_fused = on == 1;
  return ZIGP_OK;
}

int zigp_get_kron_matern_fused(zigp_ctx* c) {
  if (!c) return ZIGP_EARG;
  return c->kron_matern_fused ? 1 : 0;
}

}  // extern "C"

// ---- stage diagnostics of the Kronecker path (include/zigp_diag.h): ONE launch of a point-wise or per-point panel kernel on
// caller-supplied operands, with the grid its production callers use (kron_run_panels / kronf_run, latent_forward_panels, latent_backward) ----
namespace {
bool kron_stage_cols_ok(int64_t N, int64_t Nc) { return N >= 1 && Nc >= N && Nc % 256 == 0 && Nc <= (1 << 20); }
// device buffer of n doubles holding the stage sentinel (fill != 0) or zeros
int kron_stage_out(zigp_ctx* c, DevBuf& b, size_t n, bool sentinel) {
  ZIGP_ENSURE(c, b, n);
  ZIGP_HIP(c, hipMemsetAsync(b.p, sentinel ? ZIGP_STAGE_SENTINEL_BYTE : 0, sizeof(double) * n, c->stream));
  return 0;
}
}  // namespace

extern "C" {

int zigp_test_kron_pointwise(zigp_ctx* c, const zigp_stage_kron_pointwise* s) {
  if (!c) return ZIGP_EARG;
  if (!s || (s->lik != ZIGP_LIK_ONOFF && s->lik != ZIGP_LIK_GAUSSIAN && s->lik != ZIGP_LIK_BERNOULLI) || s->mode < 0 || s->mode > 2 ||
      (s->dev_hyp != 0 && s->dev_hyp != 1) || !kron_stage_cols_ok(s->N, s->Nc) || !s->part_f)
    return fail_arg(c, "zigp_test_kron_pointwise: bad arguments");
  const bool two = s->lik == ZIGP_LIK_ONOFF, predict = s->mode == 2, grad = s->mode == 1;
  if (two && !s->part_g) return fail_arg(c, "zigp_test_kron_pointwise: the OnOff likelihood needs part_g");
  if (!two && s->dev_hyp && predict) return fail_arg(c, "zigp_test_kron_pointwise: no step launches the heads' predict kernel on the device block");
  const int64_t N = s->N, Nc = s->Nc, ld = predict ? (s->ld_out ? s->ld_out : N) : N;
  if (predict ? (!s->out || ld < N) : (!s->Y || !s->acc)) return fail_arg(c, "zigp_test_kron_pointwise: predict needs out (ld_out >= N), the ELBO modes need Y and acc");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const bool sent = s->sentinel_out != 0;
  const int blocks = (int)(Nc / PW_THREADS), rows = two ? 9 : 4;
  DevBuf pf, pg, dy, hyp, acc, out, pt[8];
  ZIGP_TRY(stage_upload_rows(c, pf, s->part_f, 4, 4, Nc));
  if (two) ZIGP_TRY(stage_upload_rows(c, pg, s->part_g, 4, 4, Nc));
  if (s->Y) ZIGP_TRY(stage_upload_rows(c, dy, s->Y, N, N, 1));
  for (DevBuf& b : pt) ZIGP_TRY(kron_stage_out(c, b, (size_t)Nc, sent));
  ZIGP_TRY(kron_stage_out(c, acc, (size_t)blocks * KPW_ACC, sent));
  if (predict) ZIGP_TRY(kron_stage_out(c, out, (size_t)rows * ld, sent));
  KronPwArgs a;
  memset(&a, 0, sizeof(a));
  a.part_f = pf.p; a.part_g = two ? pg.p : pf.p; a.Y = s->Y ? dy.p : nullptr; a.N = N; a.Nc = Nc;
  a.knn_f = s->var0f * s->var1f; a.knn_g = s->var0g * s->var1g; a.noise = s->noise;      // as kron_run_panels forms them
  a.g_offset = s->g_offset; a.f_offset = s->f_offset; a.scale = s->scale;
  a.gm_f = grad ? pt[0].p : nullptr; a.gv_f = pt[1].p; a.dq0_f = pt[2].p; a.dq1_f = pt[3].p;
  a.gm_g = pt[4].p; a.gv_g = pt[5].p; a.dq0_g = pt[6].p; a.dq1_g = pt[7].p;
  a.acc = acc.p; a.out9 = predict ? out.p : nullptr; a.ld9 = ld; a.hyp = nullptr;
  if (s->dev_hyp) {
    // the block kronf_run stages (kf_fill_hyp); the lengthscale slots are not read by these kernels
    double H[KH_SIZE], one[MAXD];
    for (double& v : one) v = 1.0;
    const KronHostLatent hl[2] ={{{1, 1}, {nullptr, nullptr}, {one, one}, {s->var0f, s->var1f}, nullptr, nullptr},
                                {{1, 1}, {nullptr, nullptr}, {one, one}, {s->var0g, s->var1g}, nullptr, nullptr}};
    kf_fill_hyp(H, hl, two ? 2 : 1, 1, 1, s->noise);
    H[KH_FMU] = s->f_offset;                    // the slot k_fit_update writes f_mu to
    ZIGP_TRY(stage_upload_rows(c, hyp, H, 1, 1, KH_SIZE));
    a.hyp = hyp.p;
    a.knn_f = a.knn_g = a.noise = 0.0;          // a fit call leaves the by-value fields zero
    if (!two) a.f_offset = 0.0;
  }
  if (two) {
    if (predict) hipLaunchKernelGGL(k_kron_pointwise<true>, dim3(blocks), dim3(PW_THREADS), 0, c->stream, a);
    else hipLaunchKernelGGL(k_kron_pointwise<false>, dim3(blocks), dim3(PW_THREADS), 0, c->stream, a);
  } else if (predict) hipLaunchKernelGGL((k_kron_head_pointwise<true, false>), dim3(blocks), dim3(PW_THREADS), 0, c->stream, a, (int)s->lik);
  else if (s->dev_hyp) hipLaunchKernelGGL((k_kron_head_pointwise<false, true>), dim3(blocks), dim3(PW_THREADS), 0, c->stream, a, (int)s->lik);
  else hipLaunchKernelGGL((k_kron_head_pointwise<false, false>), dim3(blocks), dim3(PW_THREADS), 0, c->stream, a, (int)s->lik);
  ZIGP_HIP(c, hipGetLastError());
  if (predict) ZIGP_TRY(stage_download_rows(c, out.p, s->out, rows, ld));
  else {
    double* const host[8] = {s->gm_f, s->gv_f, s->dq0_f, s->dq1_f, s->gm_g, s->gv_g, s->dq0_g, s->dq1_g};
    for (int i = 0; i < 8; ++i) ZIGP_TRY(stage_download_rows(c, pt[i].p, host[i], 1, Nc));
    ZIGP_TRY(stage_download_rows(c, acc.p, s->acc, blocks, KPW_ACC));
  }
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

// One value-and-gradient step of the fused path through kronf_run itself, with its device buffers snapshot (KfTap, zigp_kronf.hip)
int zigp_test_kron_fused_step(zigp_ctx* c, const zigp_stage_kron_fused* s) {
  if (!c) return ZIGP_EARG;
  if (!s) return fail_arg(c, "zigp_test_kron_fused_step: bad arguments");
  ZIGP_TRY(validate_kron(c, s->p, s->lik));
  const int nlat = s->lik == ZIGP_LIK_ONOFF ? 2 : 1;
  if (s->N < 1 || !s->X || !s->Y || !s->grads || !(s->jitter >= 0)) return fail_arg(c, "zigp_test_kron_fused_step: need N >= 1 rows X, Y, grads and jitter >= 0");
  KronHostLatent kinds[2] = {};
  kron_set_kinds(c, kinds, nlat);
  if (c->kron_panels || !kf_eligible(s->p, nlat) || !kron_kinds_fused(c, kinds, nlat))
    return fail_arg(c, "zigp_test_kron_fused_step: this step does not run on the fused Kronecker kernels (grid beyond them, or zigp_set_kron_panels)");
  ZIGP_HIP(c, hipSetDevice(c->device));
  KfTap tap;
  tap.s = s;
  memset(tap.facts, 0, sizeof(tap.facts));
  for (int h = 0; h < nlat; ++h)
    if (s->lat[h].inject) ZIGP_TRY(stage_upload_rows(c, tap.inject[h], s->lat[h].inject, 4, 4, s->N));
  KronCall k = {};
  k.p = s->p; k.lik = s->lik; k.X = s->X; k.Y = s->Y; k.N = s->N; k.jitter = s->jitter; k.scale = s->scale; k.g_offset = s->g_offset; k.f_mu = s->f_mu;
  k.include_kl = s->include_kl; k.elbo_data = s->elbo_data; k.kl = s->kl; k.grads = s->grads; k.d_offset = s->d_f_mu;
  kron_call_derive(k);
  kron_set_kinds(c, k.hl, nlat);
  ZIGP_TRY(kronf_run(c, k, nullptr, &tap));
  return tap.flush(c);
}

// One value-and-gradient step of the panel path through kron_run_panels itself, with its device buffers snapshot (KpTap)
int zigp_test_kron_panel_step(zigp_ctx* c, const zigp_stage_kron_panels* s) {
  if (!c) return ZIGP_EARG;
  if (!s) return fail_arg(c, "zigp_test_kron_panel_step: bad arguments");
  ZIGP_TRY(validate_kron(c, s->p, s->lik));
  const int nlat = s->lik == ZIGP_LIK_ONOFF ? 2 : 1;
  if (s->N < 1 || !s->X || !s->Y || !s->grads || !(s->jitter >= 0)) return fail_arg(c, "zigp_test_kron_panel_step: need N >= 1 rows X, Y, grads and jitter >= 0");
  for (int h = 0; h < nlat; ++h)
    if (s->lat[h].planes_of < 0 || s->lat[h].planes_of > 3) return fail_arg(c, "zigp_test_kron_panel_step: planes_of must be 0 .. 3");
  KronHostLatent kinds[2] = {};
  kron_set_kinds(c, kinds, nlat);
  if (!c->kron_panels && kf_eligible(s->p, nlat) && kron_kinds_fused(c, kinds, nlat))
    return fail_arg(c, "zigp_test_kron_panel_step: this step runs on the fused Kronecker kernels (force the panels with zigp_set_kron_panels)");
  ZIGP_HIP(c, hipSetDevice(c->device));
  KpTap tap;
  tap.s = s;
  memset(tap.facts, 0, sizeof(tap.facts));
  for (int h = 0; h < nlat; ++h)
    if (s->lat[h].inject) ZIGP_TRY(stage_upload_rows(c, tap.inject[h], s->lat[h].inject, 4, 4, s->N));
  KronCall k = {};
  k.p = s->p; k.lik = s->lik; k.X = s->X; k.Y = s->Y; k.N = s->N; k.jitter = s->jitter; k.scale = s->scale; k.g_offset = s->g_offset; k.f_mu = s->f_mu;
  k.include_kl = s->include_kl; k.elbo_data = s->elbo_data; k.kl = s->kl; k.grads = s->grads; k.d_offset = s->d_f_mu;
  kron_call_derive(k);
  kron_set_kinds(c, k.hl, nlat);
  ZIGP_TRY(kron_run_panels(c, k, &tap));
  return tap.flush(c);
}

// The update kernel of the Kronecker fit loops through kf_fit_run itself, each step replaced by the caller's result block (KfFitTap,
// zigp_kronf.hip).  The checks are those of kron_fit_entry that do not concern rows or the data set.
int zigp_test_kron_fit_update(zigp_ctx* c, const zigp_stage_kron_fit_update* s) {
  const char* who = "zigp_test_kron_fit_update";
  if (!c) return ZIGP_EARG;
  c->fit_steps_applied = 0;
  if (!s || !s->shape || !s->lr || !s->positive || !s->x || !s->m || !s->v) return kron_refuse(c, who, "NULL argument");
  if (s->lik != ZIGP_LIK_ONOFF && s->lik != ZIGP_LIK_GAUSSIAN && s->lik != ZIGP_LIK_BERNOULLI) return kron_refuse(c, who, "unknown likelihood");
  const bool head = s->lik != ZIGP_LIK_ONOFF;
  const zigp_kron_params* p = s->shape;
  if (p->M0f <= 0 || p->M1f <= 0 || (!head && (p->M0g <= 0 || p->M1g <= 0))) return fail_arg(c, "inducing counts must be positive");
  if (p->D0 <= 0 || p->D1 <= 0 || p->D0 > MAXD || p->D1 > MAXD) return fail_arg(c, "factor dimensions must be in [1, 8]");
  if (s->n_steps <= 0 || s->n_steps > 4096 || s->t0 < 0) return kron_refuse(c, who, "need 0 < n_steps <= 4096, t0 >= 0");
  if (!(s->beta1 >= 0 && s->beta1 < 1 && s->beta2 >= 0 && s->beta2 < 1 && s->eps > 0)) return kron_refuse(c, who, "bad Adam constants");
  if (c->kron_panels || !kf_eligible(p, head ? 1 : 2))
    return kron_refuse(c, who, "this inducing grid is beyond the fused Kronecker kernels (<= 32 x <= 32 or <= 16 x <= 112 points, factor dimensions <= 7)");
  if (head && s->n_free != (int64_t)p->M0f * p->D0 + (int64_t)p->M1f * p->D1 + 2 * (int64_t)p->M0f * p->M1f + p->D0 + p->D1 + 4)
    return kron_refuse(c, who, "n_free does not match the model sizes");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const std::vector<int64_t> rows((size_t)s->n_steps, 0);      // no step runs: nothing reads a row
  KfFitCall fit = {};
  fit.name = who; fit.head = head;
  fit.lr = s->lr; fit.positive = s->positive; fit.trainable = head ? s->trainable : nullptr;
  fit.beta1 = s->beta1; fit.beta2 = s->beta2; fit.eps = s->eps;
  fit.x = s->x; fit.m = s->m; fit.v = s->v; fit.n_free = s->n_free; fit.t0 = s->t0; fit.n_steps = s->n_steps; fit.row_begin = rows.data();
  fit.batch = 1; fit.hist_data = s->elbo_data; fit.hist_kl = s->kl;
  KronCall k = {};
  k.p = p; k.lik = s->lik; k.X = k.Y = kron_no_rows; k.N = 1; k.dev_xy = true; k.scale = 1.0; k.include_kl = 1;
  kron_call_derive(k);
  kron_set_kinds(c, k.hl, k.nlat);
  k.need_grad = true;
  KfFitTap tap;
  tap.s = s; tap.nf = tap.n_img = 0; tap.taken = 0;
  memset(tap.facts, 0, sizeof(tap.facts));
  const int rc = kronf_run(c, k, &fit, nullptr, &tap);
  if (s->steps_applied) *s->steps_applied = c->fit_steps_applied;
  return rc;
}

int zigp_test_kron_kbuild(zigp_ctx* c, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, int32_t M, int32_t D, const double* X, const double* Z,
                          const double* ell, double var, double* K) {
  if (!c) return ZIGP_EARG;
  if (!kron_stage_cols_ok(N, Nc) || M <= 0 || M > 4096 || D < 1 || D > MAXD || col0 < 0 || col0 + D > ldx || !X || !Z || !ell || !K)
    return fail_arg(c, "zigp_test_kron_kbuild: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int Mq = (int)round_up(M, BM);
  DevBuf dx, dz, dk;
  ZIGP_TRY(stage_upload_rows(c, dx, X, N, N, ldx));
  ZIGP_TRY(stage_upload_rows(c, dz, Z, M, Mq, D));
  ZIGP_TRY(kron_stage_out(c, dk, (size_t)Mq * Nc, true));
  hipLaunchKernelGGL(k_kron_kbuild, dim3((unsigned)(Nc / 256), Mq / 16), dim3(256), 0, c->stream, dx.p, N, (int)ldx, (int)col0, dz.p, (int)M,
                     make_hyp(ell, var, D), dk.p, Nc);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(stage_download_rows(c, dk.p, K, Mq, Nc));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_test_kron_colsum(zigp_ctx* c, int32_t M0, int32_t M1, int64_t Nc, const double* K0, const double* A0, const double* K1, const double* A1,
                          const double* B1, const double* A0sq, const double* C1, double* part) {
  if (!c) return ZIGP_EARG;
  if (!kron_stage_cols_ok(1, Nc) || M0 <= 0 || M1 <= 0 || M0 > 4096 || M1 > 4096 || !K0 || !A0 || !K1 || !A1 || !B1 || !A0sq || !C1 || !part)
    return fail_arg(c, "zigp_test_kron_colsum: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const double* host[7] = {K0, A0, K1, A1, B1, A0sq, C1};
  const int rows[7] = {M0, M0, M1, M1, M0, M0, M0};
  DevBuf d[7], dp;
  for (int i = 0; i < 7; ++i) ZIGP_TRY(stage_upload_rows(c, d[i], host[i], rows[i], rows[i], Nc));
  ZIGP_TRY(kron_stage_out(c, dp, (size_t)4 * Nc, true));
  hipLaunchKernelGGL(k_kron_colsum, dim3((unsigned)(Nc / 256)), dim3(256), 0, c->stream, d[0].p, d[1].p, d[2].p, d[3].p, d[4].p, d[5].p, d[6].p,
                     (int)M0, (int)M1, Nc, dp.p);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(stage_download_rows(c, dp.p, part, 4, Nc));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_test_kron_da(zigp_ctx* c, int32_t M, int64_t Nc, const double* A, const double* C, const double* K, const double* gv, const double* dq,
                      double* dA, double* E) {
  if (!c) return ZIGP_EARG;
  if (!kron_stage_cols_ok(1, Nc) || M <= 0 || M > 4096 || !A || !C || !K || !gv || !dq || !dA || !E) return fail_arg(c, "zigp_test_kron_da: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int Mq = (int)round_up(M, BM);
  const int64_t pn = (int64_t)Mq * Nc;
  DevBuf da, dc, dk, dgv, ddq, oA, oE;
  ZIGP_TRY(stage_upload_rows(c, da, A, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, dc, C, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, dk, K, M, Mq, Nc));
  ZIGP_TRY(stage_upload_rows(c, dgv, gv, 1, 1, Nc)); ZIGP_TRY(stage_upload_rows(c, ddq, dq, 1, 1, Nc));
  ZIGP_TRY(kron_stage_out(c, oA, (size_t)pn, true)); ZIGP_TRY(kron_stage_out(c, oE, (size_t)pn, true));
  hipLaunchKernelGGL(k_kron_da, dim3(ceil_div(pn, 256)), dim3(256), 0, c->stream, da.p, dc.p, dk.p, dgv.p, ddq.p, Nc, pn, oA.p, oE.p);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(stage_download_rows(c, oA.p, dA, M, Nc)); ZIGP_TRY(stage_download_rows(c, oE.p, E, M, Nc));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

int zigp_test_kron_kgrad(zigp_ctx* c, int32_t M, int32_t D, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, const double* B, const double* A,
                         const double* PdA, const double* K, const double* gm, const double* dq, const double* X, const double* Z, double* krow) {
  if (!c) return ZIGP_EARG;
  if (!kron_stage_cols_ok(N, Nc) || M <= 0 || M > 4096 || D < 1 || D > MAXD || col0 < 0 || col0 + D > ldx || !B || !A || !PdA || !K || !gm || !dq ||
      !X || !Z || !krow)
    return fail_arg(c, "zigp_test_kron_kgrad: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int Mq = (int)round_up(M, BM), Wd = 2 + 2 * D;
  DevBuf db, da, dp, dk, dgm, ddq, dx, dz, dr;
  ZIGP_TRY(stage_upload_rows(c, db, B, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, da, A, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, dp, PdA, M, Mq, Nc));
  ZIGP_TRY(stage_upload_rows(c, dk, K, M, Mq, Nc));
  ZIGP_TRY(stage_upload_rows(c, dgm, gm, 1, 1, Nc)); ZIGP_TRY(stage_upload_rows(c, ddq, dq, 1, 1, Nc));
  ZIGP_TRY(stage_upload_rows(c, dx, X, N, N, ldx)); ZIGP_TRY(stage_upload_rows(c, dz, Z, M, Mq, D));
  ZIGP_TRY(stage_upload_rows(c, dr, krow, M, Mq, Wd));
  hipLaunchKernelGGL(k_kron_kgrad, dim3(Mq), dim3(256), 0, c->stream, db.p, da.p, dp.p, dk.p, dgm.p, ddq.p, dx.p, N, (int)ldx, (int)col0, dz.p, (int)M,
                     (int)D, Nc, dr.p);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(stage_download_rows(c, dr.p, krow, M, Wd));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

// The factor panel of any kind through the launch latent_forward_panels makes for it: ZIGP_KERN_RBF is zigp_test_kron_kbuild (Kd, when
// asked for, is a copy of K: K' = K), a Matern kind k_kron_kbuild_matern<KIND, Kd != NULL>.
int zigp_test_kron_kbuild_kind(zigp_ctx* c, int32_t kind, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, int32_t M, int32_t D, const double* X,
                               const double* Z, const double* ell, double var, double* K, double* Kd) {
  if (!c) return ZIGP_EARG;
  if (kind != ZIGP_KERN_RBF && kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52) return fail_arg(c, "zigp_test_kron_kbuild_kind: unknown kernel kind");
  if (!kron_stage_cols_ok(N, Nc) || M <= 0 || M > 4096 || D < 1 || D > MAXD || col0 < 0 || col0 + D > ldx || !X || !Z || !ell || !K)
    return fail_arg(c, "zigp_test_kron_kbuild_kind: bad arguments");
  if (kind == ZIGP_KERN_RBF) {
    ZIGP_TRY(zigp_test_kron_kbuild(c, N, Nc, ldx, col0, M, D, X, Z, ell, var, K));
    if (Kd) memcpy(Kd, K, sizeof(double) * (size_t)round_up(M, BM) * Nc);
    return ZIGP_OK;
  }
  ZIGP_HIP(c, hipSetDevice(c->device));
  KronFactor f;
  f.M = M; f.Mq = (int)round_up(M, BM); f.D = D; f.col0 = col0; f.var = var; f.kind = kind;
  f.ell.assign(ell, ell + D);
  DevBuf dx;
  ZIGP_TRY(stage_upload_rows(c, dx, X, N, N, ldx));
  ZIGP_TRY(stage_upload_rows(c, f.Z, Z, M, f.Mq, D));
  ZIGP_TRY(kron_stage_out(c, f.Kp, (size_t)f.Mq * Nc, true));
  if (Kd) ZIGP_TRY(kron_stage_out(c, f.Kd, (size_t)f.Mq * Nc, true));
  ZIGP_TRY(factor_kbuild_matern(c, f, dx.p, N, Nc, (int)ldx, Kd != nullptr));
  ZIGP_TRY(stage_download_rows(c, f.Kp.p, K, f.Mq, Nc));
  if (Kd) ZIGP_TRY(stage_download_rows(c, f.Kd.p, Kd, f.Mq, Nc));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

// The factor cotangent of any kind: ZIGP_KERN_RBF is zigp_test_kron_kgrad (Kd is not read), a Matern kind k_kron_kgrad_matern on K and K'.
int zigp_test_kron_kgrad_kind(zigp_ctx* c, int32_t kind, int32_t M, int32_t D, int64_t N, int64_t Nc, int32_t ldx, int32_t col0, const double* B,
                              const double* A, const double* PdA, const double* K, const double* Kd, const double* gm, const double* dq,
                              const double* X, const double* Z, double* krow) {
  if (!c) return ZIGP_EARG;
  if (kind == ZIGP_KERN_RBF) return zigp_test_kron_kgrad(c, M, D, N, Nc, ldx, col0, B, A, PdA, K, gm, dq, X, Z, krow);
  if (kind != ZIGP_KERN_MATERN32 && kind != ZIGP_KERN_MATERN52) return fail_arg(c, "zigp_test_kron_kgrad_kind: unknown kernel kind");
  if (!kron_stage_cols_ok(N, Nc) || M <= 0 || M > 4096 || D < 1 || D > MAXD || col0 < 0 || col0 + D > ldx || !B || !A || !PdA || !K || !Kd || !gm ||
      !dq || !X || !Z || !krow)
    return fail_arg(c, "zigp_test_kron_kgrad_kind: bad arguments");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const int Mq = (int)round_up(M, BM), Wd = 2 + 2 * D;
  DevBuf db, da, dp, dk, dkd, dgm, ddq, dx, dz, dr;
  ZIGP_TRY(stage_upload_rows(c, db, B, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, da, A, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, dp, PdA, M, Mq, Nc));
  ZIGP_TRY(stage_upload_rows(c, dk, K, M, Mq, Nc)); ZIGP_TRY(stage_upload_rows(c, dkd, Kd, M, Mq, Nc));
  ZIGP_TRY(stage_upload_rows(c, dgm, gm, 1, 1, Nc)); ZIGP_TRY(stage_upload_rows(c, ddq, dq, 1, 1, Nc));
  ZIGP_TRY(stage_upload_rows(c, dx, X, N, N, ldx)); ZIGP_TRY(stage_upload_rows(c, dz, Z, M, Mq, D));
  ZIGP_TRY(stage_upload_rows(c, dr, krow, M, Mq, Wd));
  hipLaunchKernelGGL(k_kron_kgrad_matern, dim3(Mq), dim3(256), 0, c->stream, db.p, da.p, dp.p, dk.p, dkd.p, dgm.p, ddq.p, dx.p, N, (int)ldx, (int)col0,
                     dz.p, (int)M, (int)D, Nc, dr.p);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(stage_download_rows(c, dr.p, krow, M, Wd));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

}  // extern "C"
