// Held-out predictive density and the moments of y (include/zigp.h "predictive density").
//
// OnOff, per test row: under q, f ~ N(fm, fv) and g ~ N(gm, gv) are independent (rows 3-6 of zigp_predict, mean function and g_offset
// applied) and y | f, g ~ N(Phi~(g) f, noise), Phi~ the link of pointwise_eval (zigp_kernels.h).  f integrates out in closed form, g by
// the caller's rule for the standard normal (nodes x_i, weights w_i > 0, sum w_i = 1):
//   Phi_i = Phi~(gm + sqrt(max(gv, 0)) x_i)
//   s_i   = noise + Phi_i^2 max(fv, 0)
//   logp  = logsumexp_i [ log w_i - 0.5 log(2 pi s_i) - 0.5 (y - Phi_i fm)^2 / s_i ]
// That finite sum is the definition; its distance from the integral belongs to the rule (tools/density_accuracy.py).
// Heads, closed form: Gaussian logp = log N(y; fm, fv + noise); Bernoulli p = the probability of k_kron_head_pointwise,
// logp = log p (y == 1) or log1p(-p).
//
// Centred (OnOff only; k_density_rows<ZIGP_LIK_ONOFF, true>, the zigp_*_centred entry points): the same N(0, 1) rule, shifted and scaled
// per row to a mode of the integrand.  With sg = sqrt(max(gv, 0)), z = (g - gm) / sg and l(u) = -0.5 log(2 pi s(u)) - 0.5 (y - u fm)^2 / s(u),
// s(u) = noise + u^2 max(fv, 0):
//   F(z)  = -z^2 / 2 + l(Phi~(gm + sg z))
//   zhat  = a local maximiser of F, by a safeguarded Newton search from z = 0 (dc_search);  tau = 1 / sqrt(-F''(zhat)), at most DC_TAU_MAX
//   z_i   = zhat + tau x_i
//   logp  = logsumexp_i [ log w_i + x_i^2 / 2 + log tau - z_i^2 / 2 + l(Phi~(gm + sg z_i)) ]
// (the change of variables z = zhat + tau x under the same rule; one node is the Laplace approximation).  Given (zhat, tau), which the
// kernel returns, that finite sum is the definition.
//
// One kernel template, k_density_rows<LIK, CENTRED>, in four instantiations (OnOff with either centre, the two heads), and one host path
// on the row-call layer of zigp_rows.h: density_rows (rows_from_host) behind the two zigp_density_rows* entries, predict_density
// (rows_from_predict) behind the four zigp_predict_density* entries, density_run behind both.  The two OnOff sums are written out side
// by side (dn_logsumexp): equal in exact arithmetic at zhat = 0, tau = 1, they differ in their rounding.  The regions of scratch2, in
// allocation order, each from a multiple of 8 doubles: the rule's table, the sum, the block partials, the (3, N) rows and -- centred --
// the (2, N) centre.  Resources on gfx950 (-Rpass-analysis=kernel-resource-usage),
// VGPRs / LDS bytes per block / waves per SIMD, no scratch anywhere: <ONOFF, false> 101 / 4128 / 4, <ONOFF, true> 130 / 6176 / 3,
// <GAUSSIAN, false> 24 / 32 / 8, <BERNOULLI, false> 28 / 32 / 8.
#include "zigp_rows.h"
#include <cmath>

using namespace zigp;

namespace zigp {

constexpr int DN_THREADS = 256;   // rows per block (one thread each); not tuned: tools/density_time.py is the measurement
constexpr int DN_MAXQ = 256;      // ZIGP_DENSITY_MAX_QUAD
static_assert(DN_MAXQ == ZIGP_DENSITY_MAX_QUAD, "include/zigp.h");

struct DensityArgs {
  const double* fm; const double* fv; const double* gm; const double* gv; const double* y;   // rows [N] (gm, gv: OnOff only)
  const double* m0; const double* m1; const double* m2;   // OnOff: gfmean, gfvar, gfmeanu of a predict block; NULL: from the four rows
  int64_t N;
  double noise;
  const double* rule;   // OnOff: x_i [n_quad], then log w_i [n_quad]; centred: then x_i^2 / 2 [n_quad]
  int n_quad;
  double* out3;         // (3, ld3): logp, ymean, yvar (nullable)
  int64_t ld3;
  double* centre2;      // centred: (2, ldc): zhat, tau (nullable)
  int64_t ldc;
  double* part;         // [gridDim.x] block sums of logp
};

constexpr double DN_LOG_2PI = 1.8378770664093454836;

__device__ __forceinline__ double dn_link(double g) {   // OnOffSVGP.py:178, as pointwise_eval writes it
  const double c1 = 1.0 - 2.e-3, c0 = 1.e-3;
  return 0.5 * (1.0 + erf(g * 0.70710678118654752440)) * c1 + c0;
}

// ---- the rule centred on each row's mode ------------------------------------------------------------------------------------------
constexpr int DC_MAX_ITER = 60;        // Newton iterations at most: a row can never spin
constexpr int DC_MAX_HALVE = 30;       // halvings of one step at most
constexpr double DC_TAU_MAX = 1.5;     // tau = 1 / sqrt(-F'') is clamped to (0, DC_TAU_MAX]
constexpr double DC_SG_FLOOR = 1.e-3;  // a step is at most one unit of g: 1 / max(sg, DC_SG_FLOOR) in z
constexpr double DC_FREE_STEP = 1.e-4; // in units of 1 / sqrt(-F''): a Newton step this small is taken unchecked (F cannot resolve it) ...
constexpr double DC_STOP_STEP = 1.e-9; // ... and one this small ends the search
constexpr double DC_INV_SQRT_2PI = 0.39894228040143267794;

struct DcRow { double fm, fvp, gm, sg, y, noise; };   // an OnOff row as both sums read it: fvp = max(fv, 0), sg = sqrt(max(gv, 0))
struct DcVal { double F, F1, F2; };

// F, F' and F'' at z:  F' = -z + sg l'(u) phi(g),  F'' = -1 + sg^2 [ l''(u) phi(g)^2 - g l'(u) phi(g) ],  phi(g) = (1 - 2e-3) N(g; 0, 1)
__device__ __forceinline__ DcVal dc_eval(const DcRow& w, double z) {
  const double g = w.gm + w.sg * z;
  const double ph = dn_link(g);
  const double dph = (1.0 - 2.e-3) * DC_INV_SQRT_2PI * exp(-0.5 * g * g);
  const double s = w.noise + ph * ph * w.fvp, r = w.y - ph * w.fm, q = ph * w.fvp;
  const double r2 = r * r, s2 = s * s;
  DcVal v;
  v.F = -0.5 * z * z + (-0.5 * (DN_LOG_2PI + log(s)) - 0.5 * r2 / s);
  const double l1 = (r * w.fm - q) / s + r2 * q / s2;
  const double l2 = -(w.fvp + w.fm * w.fm) / s + (2.0 * q * q - 4.0 * r * w.fm * q + r2 * w.fvp) / s2 - 4.0 * r2 * (q * q) / (s2 * s);
  v.F1 = -z + w.sg * l1 * dph;
  v.F2 = -1.0 + w.sg * w.sg * (l2 * dph * dph - g * l1 * dph);
  return v;
}

// The search, in registers: Newton where -F'' > 0, else a capped step along sign(F'); every step capped at one unit of g and halved until
// F does not decrease.  sg = 0 gives F' = 0 and F'' = -1 exactly: zhat = 0, tau = 1.
__device__ __forceinline__ void dc_search(const DcRow& w, double& zhat, double& tau) {
  const double cap = 1.0 / fmax(w.sg, DC_SG_FLOOR);
  double z = 0.0;
  DcVal v = dc_eval(w, z);
  for (int it = 0; it < DC_MAX_ITER; ++it) {
    const double h = -v.F2;
    const bool newton = h > 0.0;
    double step = newton ? v.F1 / h : (v.F1 > 0.0 ? cap : v.F1 < 0.0 ? -cap : 0.0);
    step = step > cap ? cap : step < -cap ? -cap : step;
    if (!(fabs(step) > 0.0)) break;   // zero or NaN
    const double unit = newton ? 1.0 / sqrt(h) : 0.0;
    const bool free_step = fabs(step) <= DC_FREE_STEP * unit, stop = fabs(step) <= DC_STOP_STEP * unit;
    bool accepted = false;
    double zn = z;
    DcVal vn = v;
    for (int k = 0; k <= DC_MAX_HALVE; ++k) {
      zn = z + step;
      vn = dc_eval(w, zn);
      if (free_step || vn.F >= v.F) { accepted = true; break; }
      step *= 0.5;
    }
    if (!accepted) break;
    z = zn; v = vn;
    if (stop) break;
  }
  const double h = -v.F2;
  zhat = z;
  tau = h > 0.0 ? fmin(1.0 / sqrt(h), DC_TAU_MAX) : 1.0;
}

// ---- the pieces of k_density_rows -------------------------------------------------------------------------------------------------
// The rule's table (COLS columns of n_quad entries) into LDS, once per block
template <int COLS>
__device__ __forceinline__ void dn_stage_rule(const DensityArgs& a, double (&tab)[COLS][DN_MAXQ]) {
  for (int i = threadIdx.x; i < a.n_quad; i += DN_THREADS)
    for (int k = 0; k < COLS; ++k) tab[k][i] = a.rule[k * a.n_quad + i];
  __syncthreads();
}

// The OnOff sum of one row over the staged rule (tab[0] = x_i, tab[1] = log w_i, centred: tab[2] = x_i^2 / 2, the nodes at zhat + tau x_i
// and lt = log tau).  Online log-sum-exp: m = the largest term so far, acc = sum exp(term - m); the first node starts it, so that no -inf
// meets -inf.
template <bool CENTRED, int COLS>
__device__ __forceinline__ double dn_logsumexp(const DcRow& w, const double (&tab)[COLS][DN_MAXQ], int n_quad, double zhat, double tau, double lt) {
  static_assert(COLS == (CENTRED ? 3 : 2), "the centred table has a third column");
  double m = 0.0, acc = 1.0;
  for (int i = 0; i < n_quad; ++i) {
    double z = tab[0][i];
    if constexpr (CENTRED) z = zhat + tau * tab[0][i];
    const double ph = dn_link(w.gm + w.sg * z);
    const double s = w.noise + ph * ph * w.fvp, r = w.y - ph * w.fm;
    double l;   // the two sums keep their own association: they differ in bits where they agree in exact arithmetic
    if constexpr (CENTRED) l = ((tab[1][i] + tab[2][i]) + lt) - 0.5 * z * z + (-0.5 * (DN_LOG_2PI + log(s)) - 0.5 * (r * r) / s);
    else l = tab[1][i] - 0.5 * (DN_LOG_2PI + log(s)) - 0.5 * (r * r) / s;
    if (i == 0) { m = l; continue; }
    const double d = l - m, e = exp(-fabs(d));
    if (d > 0.0) { acc = fma(acc, e, 1.0); m = l; } else acc += e;
  }
  return m + log(acc);
}

// ymean and yvar of an OnOff row: not the rule's business, so the same bits under either centre
__device__ __forceinline__ void dn_moments(const DensityArgs& a, int64_t n, bool valid, double fm, double fv, double gm, double gv, double y,
                                           double& ymean, double& yvar) {
  if (a.m0) {   // a predict block: ymean = gfmean, yvar = (gfvar + gfmeanu) + noise, two additions in that order
    ymean = valid ? a.m0[n] : 0.0;
    yvar = __dadd_rn(__dadd_rn(valid ? a.m1[n] : 0.0, valid ? a.m2[n] : 0.0), a.noise);
  } else {
    const PwOut o = pointwise_eval(fm, fv, gm, gv, y, a.noise);
    // the two products as the ROUNDED numbers zigp_predict stores (the empty statement pins them in registers): left to the compiler,
    // one of them is fused into the addition and yvar is an ulp away from the sum of the stored rows
    double gfvar = o.gfvar, gfmeanu = o.gfmeanu;
    asm volatile("" : "+v"(gfvar), "+v"(gfmeanu));
    ymean = o.gfmean;
    yvar = __dadd_rn(__dadd_rn(gfvar, gfmeanu), a.noise);
  }
}

// The row's three results to out3, and the block's sum of logp to part (rows n >= N add zero and are written nowhere)
__device__ __forceinline__ void dn_store(const DensityArgs& a, int64_t n, bool valid, double logp, double ymean, double yvar, double* sh) {
  if (valid && a.out3) { double* q = a.out3 + n; q[0] = logp; q[a.ld3] = ymean; q[2 * a.ld3] = yvar; }
  const double sum = block_sum<DN_THREADS / 64>(valid ? logp : 0.0, sh);
  if (threadIdx.x == 0) a.part[blockIdx.x] = sum;
}

template <int LIK, bool CENTRED>
__global__ void __launch_bounds__(DN_THREADS)
k_density_rows(DensityArgs a) {
  static_assert(LIK == ZIGP_LIK_ONOFF || LIK == ZIGP_LIK_GAUSSIAN || LIK == ZIGP_LIK_BERNOULLI, "a ZIGP_LIK_* value");
  static_assert(!CENTRED || LIK == ZIGP_LIK_ONOFF, "the heads are closed form: there is no rule to centre");
  __shared__ double sh[DN_THREADS / 64];
  const int64_t n = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
  const bool valid = n < a.N;
  const double fm = valid ? a.fm[n] : 0.0, fv = valid ? a.fv[n] : 0.0, y = valid ? a.y[n] : 0.0;
  double logp, ymean, yvar;
  if constexpr (LIK == ZIGP_LIK_ONOFF) {
    __shared__ double tab[CENTRED ? 3 : 2][DN_MAXQ];
    dn_stage_rule(a, tab);
    const double gm = valid ? a.gm[n] : 0.0, gv = valid ? a.gv[n] : 0.0;
    DcRow w;
    w.fm = fm; w.fvp = fmax(fv, 0.0); w.gm = gm; w.sg = sqrt(fmax(gv, 0.0)); w.y = y; w.noise = a.noise;
    double zhat = 0.0, tau = 1.0, lt = 0.0;
    if constexpr (CENTRED) { dc_search(w, zhat, tau); lt = log(tau); }
    logp = dn_logsumexp<CENTRED>(w, tab, a.n_quad, zhat, tau, lt);
    dn_moments(a, n, valid, fm, fv, gm, gv, y, ymean, yvar);
    if constexpr (CENTRED)
      if (valid && a.centre2) { double* q = a.centre2 + n; q[0] = zhat; q[a.ldc] = tau; }
  } else if constexpr (LIK == ZIGP_LIK_GAUSSIAN) {
    const double s = __dadd_rn(fv, a.noise), r = y - fm;
    logp = -0.5 * (DN_LOG_2PI + log(s)) - 0.5 * (r * r) / s;
    ymean = fm; yvar = s;
  } else {
    const double p = dn_link(fm * (1.0 / sqrt(1.0 + fv)));   // classifier.py:216-217, k_kron_head_pointwise
    logp = (y == 1.0) ? log(p) : log1p(-p);
    ymean = p; yvar = __dmul_rn(p, 1.0 - p);
  }
  dn_store(a, n, valid, logp, ymean, yvar, sh);
}

}  // namespace zigp

namespace {

// Everything a density call refuses that is not a pointer; touches nothing but the error text
int density_check(zigp_ctx* c, const char* who, int lik, int64_t N, double noise, const double* nodes, const double* weights, int n_quad) {
  if (lik != ZIGP_LIK_ONOFF && lik != ZIGP_LIK_GAUSSIAN && lik != ZIGP_LIK_BERNOULLI) return refuse(c, who, "lik is not a ZIGP_LIK_* value");
  if (N < 0) return refuse(c, who, "N is negative");
  if (lik != ZIGP_LIK_BERNOULLI && !(noise > 0 && std::isfinite(noise))) return refuse(c, who, "noise must be positive and finite");
  if (lik != ZIGP_LIK_ONOFF) return 0;
  if (n_quad < 1 || n_quad > DN_MAXQ) return refuse(c, who, "n_quad must be in [1, 256] (ZIGP_DENSITY_MAX_QUAD)");
  if (!nodes || !weights) return refuse(c, who, "nodes or weights is NULL");
  for (int i = 0; i < n_quad; ++i) {
    if (!std::isfinite(nodes[i])) return refuse(c, who, "nodes has a non-finite entry");
    if (!(weights[i] > 0 && std::isfinite(weights[i]))) return refuse(c, who, "weights must be positive and finite");
  }
  return 0;
}

// The tail of every density call, behind either source of rows: the regions of scratch2, the rule's table (OnOff: nodes, the logarithms
// of the weights and -- centred -- x^2 / 2), the rows kernel, the sum and the outputs.  on_device: out3 and centre2 are written in place.
int density_run(zigp_ctx* c, int lik, bool centred, const PredRows& r, double noise, const double* nodes, const double* weights, int n_quad,
                double* out3, double* centre2, bool on_device, double* sum) {
  const bool onoff = lik == ZIGP_LIK_ONOFF;
  const int64_t N = r.N;
  const int nb = ceil_div(N, DN_THREADS);
  RowArena ar(c->scratch2, "c->scratch2");
  const size_t o_rule = ar.take(onoff ? (size_t)(centred ? 3 : 2) * n_quad : 0), o_sum = ar.take(1), o_part = ar.take(nb);
  const size_t o_out = ar.take((size_t)3 * N), o_centre = ar.take(centred ? (size_t)2 * N : 0);
  ZIGP_TRY(ar.commit(c));
  if (onoff) ZIGP_TRY(upload_rule(c, ar.at(o_rule), nodes, weights, n_quad, centred ? RuleForm::X_LOGW_HALFX2 : RuleForm::X_LOGW));
  DensityArgs a{};
  a.fm = r.fm; a.fv = r.fv; a.gm = r.gm; a.gv = r.gv; a.y = r.y; a.m0 = r.m0; a.m1 = r.m1; a.m2 = r.m2;
  a.N = N; a.noise = noise; a.rule = ar.at(o_rule); a.n_quad = onoff ? n_quad : 0; a.ld3 = N; a.ldc = N; a.part = ar.at(o_part);
  a.out3 = out_target(out3, on_device, ar.at(o_out)); a.centre2 = out_target(centre2, on_device, ar.at(o_centre));
  const dim3 grid(nb), block(DN_THREADS);
  if (onoff && centred) hipLaunchKernelGGL((k_density_rows<ZIGP_LIK_ONOFF, true>), grid, block, 0, c->stream, a);
  else if (onoff) hipLaunchKernelGGL((k_density_rows<ZIGP_LIK_ONOFF, false>), grid, block, 0, c->stream, a);
  else if (lik == ZIGP_LIK_GAUSSIAN) hipLaunchKernelGGL((k_density_rows<ZIGP_LIK_GAUSSIAN, false>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_density_rows<ZIGP_LIK_BERNOULLI, false>), grid, block, 0, c->stream, a);
  ZIGP_HIP(c, hipGetLastError());
  double* hsum = nullptr;
  ZIGP_TRY(sum_partials(c, a.part, nb, ar.at(o_sum), &hsum));
  ZIGP_TRY(finish_copies(c, {{on_device ? nullptr : out3, ar.at(o_out), (size_t)3 * N}, {on_device ? nullptr : centre2, ar.at(o_centre), (size_t)2 * N}}));
  *sum = hsum[0];
  return ZIGP_OK;
}

// zigp_density_rows and zigp_density_rows_centred (who: the entry's name for the messages; centred implies lik = ZIGP_LIK_ONOFF)
int density_rows(zigp_ctx* c, const char* who, int lik, bool centred, const double* fm, const double* fv, const double* gm, const double* gv,
                 const double* y, int64_t N, double noise, const double* nodes, const double* weights, int n_quad, double* out3, double* sum,
                 double* centre2) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(density_check(c, who, lik, N, noise, nodes, weights, n_quad));
  if (!sum) return refuse(c, who, "sum is NULL");
  const bool onoff = lik == ZIGP_LIK_ONOFF;
  if (N > 0 && (!fm || !fv || !y || (onoff && (!gm || !gv)))) return refuse(c, who, "a row pointer (fm, fv, gm, gv, y) is NULL");
  if (N == 0) { *sum = 0.0; return ZIGP_OK; }
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(begin_staged_call(c));
  PredRows r;
  ZIGP_TRY(rows_from_host(c, onoff, fm, fv, gm, gv, y, N, r));
  return density_run(c, lik, centred, r, noise, nodes, weights, n_quad, out3, centre2, false, sum);
}

// The four zigp_predict_density* entries (who: the entry's name for the messages).  on_device: X (N, D), Y (N), out3 and centre2 are
// device memory, read and written in place; else they are the host's, staged through scratch and scratch2.
int predict_density(zigp_ctx* c, const char* who, const zigp_params* p, const double* X, const double* Y, int64_t N, double jitter,
                    double g_offset, const double* nodes, const double* weights, int n_quad, double* out3, double* centre2, bool centred,
                    bool on_device, double* sum) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  ZIGP_TRY(density_check(c, who, ZIGP_LIK_ONOFF, N, p->noise, nodes, weights, n_quad));
  if (!sum) return refuse(c, who, "sum is NULL");
  if (N > 0 && (!X || !Y)) return refuse(c, who, "Xnew or Ynew is NULL");
  if (N == 0) { *sum = 0.0; return ZIGP_OK; }
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device)
    ZIGP_TRY(require_device_ptrs(c, {X, Y, out3, centre2}, (std::string(who) + (centred ? ": Xnew, Ynew, out3 and centre2" : ": Xnew, Ynew and out3") +
                                                            " must be device memory of the context's GPU").c_str()));
  PredRows r;
  ZIGP_TRY(rows_from_predict(c, p, X, Y, N, jitter, g_offset, on_device, r));
  return density_run(c, ZIGP_LIK_ONOFF, centred, r, p->noise, nodes, weights, n_quad, out3, centre2, on_device, sum);
}

}  // namespace

extern "C" {

int zigp_density_rows(zigp_ctx* c, int32_t lik, const double* fm, const double* fv, const double* gm, const double* gv, const double* y,
                      int64_t N, double noise, const double* nodes, const double* weights, int32_t n_quad, double* out3, double* sum) {
  return density_rows(c, "zigp_density_rows", lik, false, fm, fv, gm, gv, y, N, noise, nodes, weights, n_quad, out3, sum, nullptr);
}

int zigp_predict_density(zigp_ctx* c, const zigp_params* p, const double* Xnew, const double* Ynew, int64_t N, double jitter, double g_offset,
                         const double* nodes, const double* weights, int32_t n_quad, double* out3, double* sum) {
  return predict_density(c, "zigp_predict_density", p, Xnew, Ynew, N, jitter, g_offset, nodes, weights, n_quad, out3, nullptr, false, false, sum);
}

int zigp_predict_density_device(zigp_ctx* c, const zigp_params* p, const double* dXnew, const double* dYnew, int64_t N, double jitter,
                                double g_offset, const double* nodes, const double* weights, int32_t n_quad, double* d_out3, double* sum) {
  return predict_density(c, "zigp_predict_density_device", p, dXnew, dYnew, N, jitter, g_offset, nodes, weights, n_quad, d_out3, nullptr, false, true, sum);
}

int zigp_density_rows_centred(zigp_ctx* c, const double* fm, const double* fv, const double* gm, const double* gv, const double* y, int64_t N,
                              double noise, const double* nodes, const double* weights, int32_t n_quad, double* out3, double* sum,
                              double* centre2) {
  return density_rows(c, "zigp_density_rows_centred", ZIGP_LIK_ONOFF, true, fm, fv, gm, gv, y, N, noise, nodes, weights, n_quad, out3, sum, centre2);
}

int zigp_predict_density_centred(zigp_ctx* c, const zigp_params* p, const double* Xnew, const double* Ynew, int64_t N, double jitter,
                                 double g_offset, const double* nodes, const double* weights, int32_t n_quad, double* out3, double* sum,
                                 double* centre2) {
  return predict_density(c, "zigp_predict_density_centred", p, Xnew, Ynew, N, jitter, g_offset, nodes, weights, n_quad, out3, centre2, true, false, sum);
}

int zigp_predict_density_centred_device(zigp_ctx* c, const zigp_params* p, const double* dXnew, const double* dYnew, int64_t N, double jitter,
                                        double g_offset, const double* nodes, const double* weights, int32_t n_quad, double* d_out3,
                                        double* sum, double* d_centre2) {
  return predict_density(c, "zigp_predict_density_centred_device", p, dXnew, dYnew, N, jitter, g_offset, nodes, weights, n_quad, d_out3, d_centre2,
                         true, true, sum);
}

}  // extern "C"
