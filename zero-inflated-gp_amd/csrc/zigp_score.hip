// Predictive CDF, quantiles and CRPS of y (include/zigp.h "predictive scores").
//
// OnOff, per test row: the predictive distribution of zigp_density.hip's fixed-centre sum, a finite Gaussian mixture over the caller's rule
// for N(0, 1) (nodes x_k, weights w_k > 0, sum w_k = 1), with sg = sqrt(max(gv, 0)) and dn_link as the density has them:
//   Phi_k = dn_link(gm + sg x_k),  mu_k = Phi_k fm,  s_k = noise + Phi_k^2 max(fv, 0),  z_k(t) = (t - mu_k) / sqrt(s_k)
//   F(t)  = sum_k w_k Phi(z_k(t)),   SF(t) = sum_k w_k Phi(-z_k(t)),   Phi(z) = erfc(-z / sqrt 2) / 2    (each its own sum: never 1 - the other)
//   quantile at p: the t with F(t) = p (p <= 1/2) or SF(t) = 1 - p (p > 1/2), inside [min_k, max_k] of mu_k + sqrt(s_k) Phi^-1(p)
//   CRPS  = sum_i w_i A(y - mu_i, s_i) - 1/2 sum_i sum_j w_i w_j A(mu_i - mu_j, s_i + s_j),
//   A(m, v) = 2 sqrt(v) phi(m / sqrt v) + m (2 Phi(m / sqrt v) - 1) = sqrt(v) (2 phi(x) + x erf(x / sqrt 2)),  x = m / sqrt(v)   (both terms >= 0)
// These finite sums are the definitions.  Gaussian head: the one-component case mu = fm, s = fv + noise (no link, no rule):
// F = Phi(z), quantile = fm + sqrt(s) Phi^-1(p), CRPS = A(y - fm, s) - sqrt(s / pi).  The Bernoulli head has no density and is refused.
// The rule is the fixed one only: a rule that moves with y (centre = 'mode') does not define one distribution per row.
//
// Layout of k_score_rows<ZIGP_LIK_ONOFF, G>: G lanes per row, 256 / G rows per block of 256 threads.  G = 64, one wave per row: lane l
// owns the nodes l, l + 64, l + 128, l + 192 (mu, s, sqrt s, w in registers); F, SF and the density are sums over the own nodes and a
// cross-lane tree, and the quantile search is wave-uniform.  For the pair sum the row's (mu, s, w) sit in a per-row LDS table (6 KB,
// 24 KB per block); the n (n - 1) / 2 pairs i < j are dealt to the G lanes as one flat list -- item e is the pair (i, i + d mod n) with
// i = e mod n, d = e / n + 1 (every unordered pair exactly once, d <= n / 2) -- so no lane idles in the O(n^2) part at any n; the
// diagonal is A(0, 2 s_i) = 2 sqrt(s_i / pi) in closed form.  Small rules would leave lanes idle in the O(n) sums (the CDF and the search):
// a rule of at most SC_HALF_MAXQ = 32 nodes runs G = 32, two rows per wave and one node per lane (the two halves of a wave search on their
// own: the loop diverges between them, every shuffle stays inside a half).  Chosen by tools/score_time.py (profiles/score_time.log), cfg2
// shape, 20 nodes, ms per call over predict_device, half a wave against a whole one (ZIGP_SCORE_WAVE_PER_ROW=1): CDF pair +0.083 against
// +0.181, with 3 levels +0.930 against +1.534, with the CRPS +1.040 against +1.694 (window spreads at most 0.058).
// k_score_rows<ZIGP_LIK_GAUSSIAN, 64>: one thread per row, 256 rows per block, closed form.
//
// One fixed association per sum, the same bits on every call, wherever the row stands and whatever N is:
//   * a lane adds its own nodes in the order l, l + G, ... (fma onto the running sum), its pairs in the order e = l, l + G, ...;
//   * the row's lanes are added by the xor tree of sc_sum (offsets G / 2, ..., 1);
//   * CRPS = [tree of the lanes' sum_k w_k A(y - mu_k, s_k)] - [tree of the lanes' (pairs + sum_k w_k^2 sqrt(s_k / pi))];
//   * the block's sum of CRPS adds its rows in row order; k_sum_partials adds the blocks (its own fixed order).
// Quantile search (sc_quantile): r(t) = F(t) - p or (1 - p) - SF(t), increasing, r' = the density; bracket [lo, hi] kept around the sign
// change of r; a Newton step where it lands strictly inside and shrinks fast enough, else the midpoint; ends when the step no longer
// changes t or the bracket is one ulp wide, after SC_MAX_ITER evaluations at the latest.  Phi^-1(p) comes from the host (sc_ndtri).
// Resources on gfx950 (-Rpass-analysis=kernel-resource-usage), VGPRs / LDS bytes per block / waves per SIMD, no scratch:
// <ONOFF, 64> 118 / 24608 / 4, <ONOFF, 32> 98 / 6208 / 4, <GAUSSIAN, 64> 30 / 32 / 8.
#include "zigp_rows.h"
#include <cmath>
#include <cstdlib>

using namespace zigp;

namespace zigp {

constexpr int SC_THREADS = 256;             // threads per block
constexpr int SC_HALF_MAXQ = 32;            // OnOff: a rule of at most this many nodes gives a row half a wave (G = 32), a larger one a whole wave (G = 64)
template <int G> struct ScGeom {            // G lanes per row: rows per block, nodes per lane at most, entries of a row's table column
  static_assert(G == 64 || G == 32, "a wave or half a wave per row");
  static constexpr int ROWS = SC_THREADS / G, SLOTS = G == 64 ? DN_MAXQ / 64 : 1, TAB = G * SLOTS;
};
constexpr int SC_MAX_ITER = 128;            // evaluations of one quantile search at most: a row can never spin
constexpr int SC_MAXL = 16;                 // ZIGP_SCORE_MAX_LEVELS
static_assert(SC_MAXL == ZIGP_SCORE_MAX_LEVELS, "include/zigp.h");
constexpr double SC_INV_SQRT2 = 0.70710678118654752440, SC_INV_SQRT_PI = 0.56418958354775628695;

struct ScoreArgs {
  const double* fm; const double* fv; const double* gm; const double* gv; const double* y;   // rows [N] (gm, gv: OnOff only; y nullable)
  int64_t N;
  double noise;
  const double* rule;   // OnOff: x_k [n_quad], then w_k [n_quad]
  int n_quad;
  int n_levels;
  double lev_q[SC_MAXL];     // p (p <= 1/2) or 1 - p: the probability of the smaller tail
  double lev_z[SC_MAXL];     // Phi^-1(p)
  int lev_lower[SC_MAXL];    // p <= 1/2: the search solves F = q; else SF = q
  double* cdf2;         // (2, ld): F(y), SF(y) (nullable)
  double* quant;        // (n_levels, ld) (nullable)
  double* crps;         // [N] (nullable)
  int64_t ld;
  int want_crps;        // the CRPS is computed: for crps, for part, or both
  double* part;         // [gridDim.x] block sums of the CRPS (want_crps)
};

template <int SLOTS> struct ScNodes { double mu[SLOTS], s[SLOTS], sd[SLOTS], w[SLOTS]; };   // a lane's own nodes (w = 0 past n_quad)

// The sum over the G lanes of a row by the xor tree (offsets G / 2, ..., 1; G = 64: wave_sum's tree); the same value in each of them
template <int G>
__device__ __forceinline__ double sc_sum(double v) {
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double sc_A(double m, double v) {
  const double sd = sqrt(v), x = m / sd;
  return sd * (2.0 * DC_INV_SQRT_2PI * exp(-0.5 * x * x) + x * erf(x * SC_INV_SQRT2));
}

// sign = +1: F(t);  sign = -1: SF(t);  PDF: also the density sum_k w_k phi(z_k) / sqrt(s_k).  The same value in every lane.
template <bool PDF, int G>
__device__ __forceinline__ double sc_tail(const ScNodes<ScGeom<G>::SLOTS>& q, int n, int lane, double t, double sign, double& pdf) {
  double acc = 0.0, d = 0.0;
#pragma unroll
  for (int k = 0; k < ScGeom<G>::SLOTS; ++k)
    if (lane + G * k < n) {
      const double z = (t - q.mu[k]) / q.sd[k];
      acc = fma(q.w[k], 0.5 * erfc(-sign * z * SC_INV_SQRT2), acc);
      if constexpr (PDF) d = fma(q.w[k], DC_INV_SQRT_2PI * exp(-0.5 * z * z) / q.sd[k], d);
    }
  if constexpr (PDF) pdf = sc_sum<G>(d);
  return sc_sum<G>(acc);
}

// The quantile at one level: q = the smaller tail's probability, zp = Phi^-1(p), lower = (p <= 1/2).  Uniform over the row's G lanes.
template <int G>
__device__ __forceinline__ double sc_quantile(const ScNodes<ScGeom<G>::SLOTS>& nd, int n, int lane, double q, double zp, bool lower) {
  double lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int k = 0; k < ScGeom<G>::SLOTS; ++k)
    if (lane + G * k < n) {
      const double c = fma(nd.sd[k], zp, nd.mu[k]);
      lo = fmin(lo, c); hi = fmax(hi, c);
    }
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, 64)); hi = fmax(hi, __shfl_xor(hi, o, 64)); }
  const double sign = lower ? 1.0 : -1.0;
  double t = lo + 0.5 * (hi - lo), dxold = hi - lo, dx = dxold;
  if (!(lo < t && t < hi)) return lo;   // one component, or all of them equal: the closed form
  for (int it = 0; it < SC_MAX_ITER; ++it) {
    double pdf;
    const double tail = sc_tail<true, G>(nd, n, lane, t, sign, pdf);
    const double r = lower ? tail - q : q - tail;   // increasing in t
    if (r == 0.0) break;
    if (r < 0.0) lo = t; else hi = t;
    const double newton = t - r / pdf;
    const bool use = newton > lo && newton < hi && fabs(2.0 * r) <= fabs(dxold * pdf);   // false on NaN
    const double tn = use ? newton : lo + 0.5 * (hi - lo);
    dxold = dx; dx = tn - t;
    if (tn == t || !(lo < tn && tn < hi)) break;   // the step changes nothing, or the bracket is one ulp wide
    t = tn;
  }
  return t;
}

template <int LIK, int G>
__global__ void __launch_bounds__(SC_THREADS)
k_score_rows(ScoreArgs a) {
  static_assert(LIK == ZIGP_LIK_ONOFF || LIK == ZIGP_LIK_GAUSSIAN, "the Bernoulli head has no density");
  if constexpr (LIK == ZIGP_LIK_ONOFF) {
    constexpr int ROWS = ScGeom<G>::ROWS, SLOTS = ScGeom<G>::SLOTS;
    __shared__ double tab[ROWS][3][ScGeom<G>::TAB];   // per row: mu, s, w
    __shared__ double shc[ROWS];
    const int lane = threadIdx.x & (G - 1), wv = threadIdx.x / G, n = a.n_quad;   // n <= ScGeom<G>::TAB (score_run)
    const int64_t row = (int64_t)blockIdx.x * ROWS + wv;
    const bool valid = row < a.N;
    const double fm = valid ? a.fm[row] : 0.0, fvp = fmax(valid ? a.fv[row] : 0.0, 0.0), gm = valid ? a.gm[row] : 0.0;
    const double sg = sqrt(fmax(valid ? a.gv[row] : 0.0, 0.0)), y = (valid && a.y) ? a.y[row] : 0.0;
    ScNodes<SLOTS> nd;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int i = lane + G * k;
      const bool on = i < n;
      const double ph = dn_link(gm + sg * (on ? a.rule[i] : 0.0));
      nd.mu[k] = ph * fm; nd.s[k] = a.noise + ph * ph * fvp; nd.sd[k] = sqrt(nd.s[k]); nd.w[k] = on ? a.rule[n + i] : 0.0;
      if (a.want_crps && on) { tab[wv][0][i] = nd.mu[k]; tab[wv][1][i] = nd.s[k]; tab[wv][2][i] = nd.w[k]; }
    }
    __syncthreads();
    if (valid) {
      if (a.cdf2) {
        double unused;
        const double F = sc_tail<false, G>(nd, n, lane, y, 1.0, unused), SF = sc_tail<false, G>(nd, n, lane, y, -1.0, unused);
        if (lane == 0) { a.cdf2[row] = F; a.cdf2[a.ld + row] = SF; }
      }
      if (a.quant)
        for (int l = 0; l < a.n_levels; ++l) {
          const double t = sc_quantile<G>(nd, n, lane, a.lev_q[l], a.lev_z[l], a.lev_lower[l] != 0);
          if (lane == 0) a.quant[(int64_t)l * a.ld + row] = t;
        }
    }
    if (a.want_crps) {
      double crps = 0.0;
      if (valid) {
        double t1 = 0.0, t2 = 0.0;
        const int P = n * (n - 1) / 2;
        for (int e = lane; e < P; e += G) {
          const int dd = e / n, i = e - dd * n;
          int j = i + dd + 1;
          if (j >= n) j -= n;
          t2 = fma(tab[wv][2][i] * tab[wv][2][j], sc_A(tab[wv][0][i] - tab[wv][0][j], tab[wv][1][i] + tab[wv][1][j]), t2);
        }
#pragma unroll
        for (int k = 0; k < SLOTS; ++k)
          if (lane + G * k < n) {
            t1 = fma(nd.w[k], sc_A(y - nd.mu[k], nd.s[k]), t1);
            t2 = fma(nd.w[k] * nd.w[k], nd.sd[k] * SC_INV_SQRT_PI, t2);
          }
        crps = sc_sum<G>(t1) - sc_sum<G>(t2);
        if (lane == 0 && a.crps) a.crps[row] = crps;
      }
      if (lane == 0) shc[wv] = crps;
      __syncthreads();
      if (threadIdx.x == 0) {
        double s = shc[0];
#pragma unroll
        for (int w = 1; w < ROWS; ++w) s += shc[w];
        a.part[blockIdx.x] = s;
      }
    }
  } else {
    __shared__ double sh[SC_THREADS / 64];
    const int64_t row = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const bool valid = row < a.N;
    const double fm = valid ? a.fm[row] : 0.0, s = __dadd_rn(valid ? a.fv[row] : 1.0, a.noise), y = (valid && a.y) ? a.y[row] : 0.0;
    const double sd = sqrt(s);
    if (valid && a.cdf2) {
      const double z = (y - fm) / sd;
      a.cdf2[row] = 0.5 * erfc(-z * SC_INV_SQRT2); a.cdf2[a.ld + row] = 0.5 * erfc(z * SC_INV_SQRT2);
    }
    if (valid && a.quant)
      for (int l = 0; l < a.n_levels; ++l) a.quant[(int64_t)l * a.ld + row] = fma(sd, a.lev_z[l], fm);
    if (a.want_crps) {
      const double crps = valid ? sc_A(y - fm, s) - sd * SC_INV_SQRT_PI : 0.0;
      if (valid && a.crps) a.crps[row] = crps;
      const double sum = block_sum<SC_THREADS / 64>(crps, sh);
      if (threadIdx.x == 0) a.part[blockIdx.x] = sum;
    }
  }
}

}  // namespace zigp

namespace {

// Lanes per OnOff row: half a wave for a rule of at most SC_HALF_MAXQ nodes, else a whole one.  ZIGP_SCORE_WAVE_PER_ROW=1 in the
// environment gives every rule a whole wave: the other arm of tools/score_time.py.
int score_group(int n_quad) {
  const char* e = getenv("ZIGP_SCORE_WAVE_PER_ROW");
  return n_quad <= SC_HALF_MAXQ && !(e && e[0] == '1') ? 32 : 64;
}

// Phi^-1(q) for q in (0, 1/2]: Acklam's rational start (relative error 1.2e-9), then Halley steps on erfc, whose relative accuracy
// holds in the tail
double sc_ndtri_lower(double q) {
  static const double A[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  static const double B[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01};
  static const double Cc[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  static const double Dd[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
  double x;
  if (q < 0.02425) {
    const double u = sqrt(-2.0 * log(q));
    x = (((((Cc[0] * u + Cc[1]) * u + Cc[2]) * u + Cc[3]) * u + Cc[4]) * u + Cc[5]) / ((((Dd[0] * u + Dd[1]) * u + Dd[2]) * u + Dd[3]) * u + 1.0);
  } else {
    const double u = q - 0.5, r = u * u;
    x = (((((A[0] * r + A[1]) * r + A[2]) * r + A[3]) * r + A[4]) * r + A[5]) * u / (((((B[0] * r + B[1]) * r + B[2]) * r + B[3]) * r + B[4]) * r + 1.0);
  }
  for (int it = 0; it < 3; ++it) {
    const double e = 0.5 * erfc(-x * 0.70710678118654752440) - q;
    const double u = e * 2.5066282746310005024 * exp(0.5 * x * x);
    x -= u / (1.0 + 0.5 * x * u);
  }
  return x;
}

// Everything a score call refuses that is not a row pointer; touches nothing but the error text
int score_check(zigp_ctx* c, const char* who, int lik, int64_t N, double noise, const double* nodes, const double* weights, int n_quad,
                const double* levels, int n_levels, bool have_y, const double* cdf2, const double* quant, const double* crps, const double* crps_sum) {
  if (lik == ZIGP_LIK_BERNOULLI)
    return refuse(c, who, "the Bernoulli head has no density, so no CDF, quantile or CRPS: its CRPS is the Brier score (ymean - y)^2 of zigp_density_rows");
  ZIGP_TRY(density_check(c, who, lik, N, noise, nodes, weights, n_quad));
  if (n_levels < 0 || n_levels > SC_MAXL) return refuse(c, who, "n_levels must be in [0, 16] (ZIGP_SCORE_MAX_LEVELS)");
  if (n_levels == 0 && (levels || quant)) return refuse(c, who, "n_levels is 0, so levels and quant must be NULL");
  if (n_levels > 0 && (!levels || !quant)) return refuse(c, who, "levels or quant is NULL");
  for (int l = 0; l < n_levels; ++l)
    if (!(levels[l] > 0.0 && levels[l] < 1.0)) return refuse(c, who, "levels must be finite and strictly inside (0, 1)");
  if (!have_y && (cdf2 || crps || crps_sum)) return refuse(c, who, "y (Ynew) is NULL, so cdf2, crps and crps_sum must be NULL");
  return 0;
}

// The tail of every score call, behind either source of rows (zigp_rows.h): the regions of scratch2, the rule's table (OnOff: nodes, then
// weights), the levels into the arguments, the rows kernel, the sum where the CRPS is asked for, and the outputs.  on_device: cdf2, quant
// and crps are written in place.  The regions, in allocation order, each from a multiple of 8 doubles: the rule's table, the sum, the block
// partials, the (2, N) CDF pair, the (n_levels, N) quantiles, the N CRPS values -- from 0, like a density call's: neither outlives its call.
int score_run(zigp_ctx* c, int lik, const PredRows& r, double noise, const double* nodes, const double* weights, int n_quad, const double* levels,
              int n_levels, double* cdf2, double* quant, double* crps, bool on_device, double* crps_sum) {
  const bool onoff = lik == ZIGP_LIK_ONOFF;
  const int64_t N = r.N;
  const int group = onoff ? score_group(n_quad) : 0;
  const int nb = ceil_div(N, !onoff ? SC_THREADS : group == 32 ? ScGeom<32>::ROWS : ScGeom<64>::ROWS);
  RowArena ar(c->scratch2, "c->scratch2");
  const size_t o_rule = ar.take(onoff ? (size_t)2 * n_quad : 0), o_sum = ar.take(1), o_part = ar.take(nb);
  const size_t o_cdf = ar.take((size_t)2 * N), o_quant = ar.take((size_t)n_levels * N), o_crps = ar.take(N);
  ZIGP_TRY(ar.commit(c));
  if (onoff) ZIGP_TRY(upload_rule(c, ar.at(o_rule), nodes, weights, n_quad, RuleForm::X_W));
  ScoreArgs a{};
  a.fm = r.fm; a.fv = r.fv; a.gm = r.gm; a.gv = r.gv; a.y = r.y;
  a.N = N; a.noise = noise; a.rule = ar.at(o_rule); a.n_quad = onoff ? n_quad : 0; a.n_levels = n_levels; a.ld = N; a.part = ar.at(o_part);
  for (int l = 0; l < n_levels; ++l) {
    const bool lower = levels[l] <= 0.5;
    const double q = lower ? levels[l] : 1.0 - levels[l], z = sc_ndtri_lower(q);   // 1 - p is exact for p > 1/2
    a.lev_q[l] = q; a.lev_z[l] = lower ? z : -z; a.lev_lower[l] = lower ? 1 : 0;
  }
  a.cdf2 = out_target(cdf2, on_device, ar.at(o_cdf)); a.quant = out_target(quant, on_device, ar.at(o_quant));
  a.crps = out_target(crps, on_device, ar.at(o_crps));
  a.want_crps = (crps || crps_sum) ? 1 : 0;
  const dim3 grid(nb), block(SC_THREADS);
  if (group == 32) hipLaunchKernelGGL((k_score_rows<ZIGP_LIK_ONOFF, 32>), grid, block, 0, c->stream, a);
  else if (onoff) hipLaunchKernelGGL((k_score_rows<ZIGP_LIK_ONOFF, 64>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_score_rows<ZIGP_LIK_GAUSSIAN, 64>), grid, block, 0, c->stream, a);
  ZIGP_HIP(c, hipGetLastError());
  double* hsum = nullptr;
  if (a.want_crps) ZIGP_TRY(sum_partials(c, a.part, nb, ar.at(o_sum), &hsum));
  ZIGP_TRY(finish_copies(c, {{on_device ? nullptr : cdf2, ar.at(o_cdf), (size_t)2 * N}, {on_device ? nullptr : quant, ar.at(o_quant), (size_t)n_levels * N},
                             {on_device ? nullptr : crps, ar.at(o_crps), (size_t)N}}));
  if (crps_sum) *crps_sum = hsum[0];
  return ZIGP_OK;
}

int score_rows(zigp_ctx* c, const char* who, int lik, const double* fm, const double* fv, const double* gm, const double* gv, const double* y,
               int64_t N, double noise, const double* nodes, const double* weights, int n_quad, const double* levels, int n_levels,
               double* cdf2, double* quant, double* crps, double* crps_sum) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(score_check(c, who, lik, N, noise, nodes, weights, n_quad, levels, n_levels, y != nullptr, cdf2, quant, crps, crps_sum));
  const bool onoff = lik == ZIGP_LIK_ONOFF;
  if (N > 0 && (!fm || !fv || (onoff && (!gm || !gv)))) return refuse(c, who, "a row pointer (fm, fv, gm, gv) is NULL");
  if (N == 0) { if (crps_sum) *crps_sum = 0.0; return ZIGP_OK; }
  if (!cdf2 && !quant && !crps && !crps_sum) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(begin_staged_call(c));
  PredRows r;
  ZIGP_TRY(rows_from_host(c, onoff, fm, fv, gm, gv, y, N, r));
  return score_run(c, lik, r, noise, nodes, weights, n_quad, levels, n_levels, cdf2, quant, crps, false, crps_sum);
}

// The two zigp_predict_scores* entries.  on_device: X (N, D), Y (N) and the three outputs are device memory, read and written in place;
// else they are the host's, staged through scratch and scratch2.
int predict_scores(zigp_ctx* c, const char* who, const zigp_params* p, const double* X, const double* Y, int64_t N, double jitter, double g_offset,
                   const double* nodes, const double* weights, int n_quad, const double* levels, int n_levels, double* cdf2, double* quant,
                   double* crps, bool on_device, double* crps_sum) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(validate_params(c, p));
  ZIGP_TRY(score_check(c, who, ZIGP_LIK_ONOFF, N, p->noise, nodes, weights, n_quad, levels, n_levels, Y != nullptr, cdf2, quant, crps, crps_sum));
  if (N > 0 && !X) return refuse(c, who, "Xnew is NULL");
  if (N == 0) { if (crps_sum) *crps_sum = 0.0; return ZIGP_OK; }
  if (!cdf2 && !quant && !crps && !crps_sum) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device)
    ZIGP_TRY(require_device_ptrs(c, {X, Y, cdf2, quant, crps},
                                 (std::string(who) + ": Xnew, Ynew, cdf2, quant and crps must be device memory of the context's GPU").c_str()));
  PredRows r;
  ZIGP_TRY(rows_from_predict(c, p, X, Y, N, jitter, g_offset, on_device, r));
  return score_run(c, ZIGP_LIK_ONOFF, r, p->noise, nodes, weights, n_quad, levels, n_levels, cdf2, quant, crps, on_device, crps_sum);
}

}  // namespace

extern "C" {

int zigp_score_rows(zigp_ctx* c, int32_t lik, const double* fm, const double* fv, const double* gm, const double* gv, const double* y,
                    int64_t N, double noise, const double* nodes, const double* weights, int32_t n_quad, const double* levels, int32_t n_levels,
                    double* cdf2, double* quant, double* crps, double* crps_sum) {
  return score_rows(c, "zigp_score_rows", lik, fm, fv, gm, gv, y, N, noise, nodes, weights, n_quad, levels, n_levels, cdf2, quant, crps, crps_sum);
}

int zigp_predict_scores(zigp_ctx* c, const zigp_params* p, const double* Xnew, const double* Ynew, int64_t N, double jitter, double g_offset,
                        const double* nodes, const double* weights, int32_t n_quad, const double* levels, int32_t n_levels, double* cdf2,
                        double* quant, double* crps, double* crps_sum) {
  return predict_scores(c, "zigp_predict_scores", p, Xnew, Ynew, N, jitter, g_offset, nodes, weights, n_quad, levels, n_levels, cdf2, quant, crps,
                        false, crps_sum);
}

int zigp_predict_scores_device(zigp_ctx* c, const zigp_params* p, const double* dXnew, const double* dYnew, int64_t N, double jitter,
                               double g_offset, const double* nodes, const double* weights, int32_t n_quad, const double* levels,
                               int32_t n_levels, double* d_cdf2, double* d_quant, double* d_crps, double* crps_sum) {
  return predict_scores(c, "zigp_predict_scores_device", p, dXnew, dYnew, N, jitter, g_offset, nodes, weights, n_quad, levels, n_levels, d_cdf2,
                        d_quant, d_crps, true, crps_sum);
}

}  // extern "C"
