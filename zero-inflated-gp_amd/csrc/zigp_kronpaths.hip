// Posterior sample paths of the Kronecker (space x time) model and its heads (include/zigp_kronpaths.h).
//
// Per latent h, test row n and sample s this finite sum is the definition (zigp_kron_path_rows computes it and nothing else):
//   out[h][s][n] = shift_h
//                + sum_{i < M0} sum_{j < M1} V_h[i M1 + j][s] ( k0_h(x_n[0:D0], z0_i) k1_h(x_n[D0:D0+D1], z1_j) )
//                + sum_{r < R} amp_h[r][s] cos( sum_d omega_h[r][d] x[n][d] + phase_h[r] )
// k_q is the element function of k_kron_kbuild (zigp_kron.hip) as it is -- inputs times 1 / ell_d, r2 by fused multiply-adds in
// ascending d, var exp(-r2 / 2) with its branch for subnormal results -- so a path and zigp_kron_predict agree on what k is.  The
// product k0 k1 is rounded once.
//
// k_kron_path_rows<D, NST, RT>, D = D0 + D1 (D0 is a run-time split): the product of k_path_rows (zigp_paths.hip) -- a 16 x (M0 M1 + R) by
// (M0 M1 + R) x rows product per tile of 16 samples on v_mfma_f64_16x16x4_f64, A = weights from a [sample tile][feature][16] table, B =
// features in registers, one per lane and instruction, D stored as 128-byte runs of out[s][n ...] -- behind a new stage:
//   stage 1  a wave owns RT = 2 or 1 tiles of 16 rows.  For each tile it evaluates the M0 + M1 factor values of its rows, (M0 + M1p) 16
//            evaluations spread over the 64 lanes (lane l: row l & 15, points (l >> 4) + 4 k), x and z read from global memory with
//            run-time-D loops, and writes them to its own LDS region as [m][16 rows]: k0 first, then k1 (M1p = M1 padded to a
//            multiple of 4; the padding holds 0).
//   stage 2  B of grid point (i, j) and row l & 15 = k0[i][l & 15] k1[j][l & 15]: one ds_read_b64 of k1 and one of k0 per instruction
//            and row tile, and one multiply.  Lane l reads the double at (64 jgroup + l) of the k1 region: a wave reads 512 contiguous
//            bytes, every bank once per pass; the k0 read is 16 distinct doubles, each broadcast to 4 lanes.  The groups of four run
//            as one flat loop over (i, jgroup), so the weights of the next 8 / NST groups are read from the table while the current
//            ones multiply: with one or two waves per SIMD nothing else hides that read.
// M0 + M1 exponentials per row instead of M0 M1.
// LDS: a wave's region is RT (M0 + M1p) 128 bytes (the larger latent's), a block is as many waves (4, 2 or 1) as fit 64 KiB of the CU's
// 160.  Two row tiles a wave share every weight read, so RT = 2 where four such waves fit a block (M0 + M1p <= 64), else RT = 1:
//   32 x 32: RT 2, 16 KiB a wave, 4 waves, 64 KiB a block -> 2 blocks a CU, 2 waves per SIMD;  10 x 100: RT 1, 13.75 KiB, 4 waves, 55 KiB
//   -> 2 blocks, 2 waves per SIMD;  128 x 128 (the limit): RT 1, 32 KiB, 2 waves -> 2 blocks, 1 wave per SIMD.  With RT 2 everywhere the
//   10 x 100 grid ran one wave per SIMD and lost to the expanded-grid call (profiles/kron_paths_time.log, first run).
// One summation order per element: the accumulator starts at +0, takes the groups of four grid points -- one i per group, ascending j
// inside ascending i -- then the groups of four cosines in ascending r; shift is added last.  A padded feature adds an exact 0 * finite.
// An element's bits do not depend on N, on the row's position, on S, on the sample's column, on NST, on the other latent or on the call.
// Resources (-Rpass-analysis=kernel-resource-usage): DESIGN.md section 10e; no instantiation uses scratch.
//
// zigp_kron_sample_paths / zigp_kron_head_sample_paths: per latent omega = omega0 / [ell0 | ell1], amp = a sqrt(2 var0 var1 / R); f_Z =
// the kernel above at the M0 M1 grid points (i, j) with the cosines alone; rhs_s = U + S o E_s - F_Z,s as M0 x M1 matrices;
// V_s = W0^T (W0 rhs_s W1^T) W1 with W_p = L_p^-1 of the call's own factor forward stage (factor_forward of zigp_kron.hip: K_p + jitter I),
// by k_kp_left / k_kp_right (one thread per element, k ascending; the refinement step V += K0^-1 (rhs - K0 V K1) K1^-1 was built and measured
// and is compiled out: the note above kp_elementwise_grid); then the kernel at Xnew, f_mu on f, g_offset on g, gf = dn_link(g) f by k_path_gf; the Bernoulli head's
// second plane is dn_link(f + f_mu) (the reference's probit link with its 1e-3 clamp, classifier.py:216-217).
#include "zigp_rows.h"
#include <cmath>
#include <cstdlib>

using namespace zigp;

namespace zigp {

constexpr int KP_RT = 2;                 // 16-row tiles per wave on the grids that leave room for them (kp_launch), else 1
constexpr int KP_MAXM = 128;             // inducing points per factor
constexpr int KP_LDS_BYTES = 65536;      // a block's LDS
static_assert((KP_MAXM + KP_MAXM) * 16 * 8 * 2 <= KP_LDS_BYTES, "two one-tile waves at the limit fit a block's LDS");

struct KpLat {
  const double* X; int64_t N;           // rows (N, D0 + D1)
  const double* Z0; const double* Z1;   // (M0, D0), (M1, D1)
  const double* omega; const double* phase;   // (R4, D), (R4); zeros behind R
  const double* tab;                    // [sample tile][F][16] weights: grid points (i, j) at i M1p + j in [0, coff), cosines [coff, coff + R4)
  double* out; int64_t ldo;             // out[s * ldo + n]
  int M0, M1, M1p, R4, F, coff, S, D0, D1;
  int kinds;                            // kind0 + 4 kind1 (ZIGP_KERN_*; 0: RBF x RBF), read by k_kron_path_rows_kinds alone.  It fills the padding
                                        // behind the nine ints: the record's size and every other offset are what the RBF kernels were built with
  double inv_ell[MAXD];                 // 1 / ell0 (D0), then 1 / ell1 (D1)
  double var0, var1, shift;
};
struct KpArgs { KpLat lat[2]; int ntile; int wave_doubles; };   // ntile: sample tiles in the table, a multiple of NST; a wave's LDS region
static_assert(sizeof(KpLat) == 200 && sizeof(KpArgs) == 408, "the kernel arguments of the RBF path kernels keep their layout");

// the element of k_kron_kbuild from its r2: var exp(-r2 / 2), with that kernel's branch for subnormal results
__device__ __forceinline__ double kp_value_of_r2(double r2, double var) {
  const double a = -0.5 * r2;
  double v = var * exp(a);
  if (v < 0x1p-1021) { const double e = exp(0.5 * a); v = (var * e) * e; }
  return v;
}

// Stage 1 for one factor and one row tile: dst[m][16 rows], m < Mp, of the points Z (M, Dq); rows m >= M hold 0.  A lane takes the points
// g, g + 4, ...; four of them go through the distance loop together, so their reads of Z are in flight at once (r2 itself is
// k_kron_kbuild's: (z / ell - x / ell)^2 by fused multiply-adds from 0 in ascending d).
__device__ __forceinline__ void kp_stage1(const double* __restrict__ xrow, const double* __restrict__ Z, const double* inv_ell, int Dq, double var,
                                          int M, int Mp, double* dst, int g, int i16) {
  for (int m0 = g; m0 < Mp; m0 += 16) {
    double r2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < Dq; ++d) {
      const double ie = inv_ell[d], xs = xrow[d] * ie;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = min(m0 + 4 * u, M - 1);      // a point behind M is read as the last one and not used
        const double t = Z[(size_t)m * Dq + d] * ie - xs;
        r2[u] = fma(t, t, r2[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + 4 * u;
      if (m < Mp) dst[m * 16 + i16] = m < M ? kp_value_of_r2(r2[u], var) : 0.0;
    }
  }
}

// kp_stage1 with the factor's kind (zigp_set_kron_kernel / zigp_kron_path_latent.kinds) as a run-time switch: RBF is kp_value_of_r2, a
// Matern kind the element of k_kron_kbuild_matern (kron_matern_elem, zigp_kron.hip) from the same r2.  Stage 1 is M0 + M1 values a row,
// off the MFMA loop.
__device__ __forceinline__ double kp_value_of_kind(int kind, double r2, double var) {
  double k, kd = 0.0;
  if (kind == KERN_RBF) return kp_value_of_r2(r2, var);
  if (kind == KERN_M32) kron_matern_elem<KERN_M32, false>(var, r2, k, kd);
  else kron_matern_elem<KERN_M52, false>(var, r2, k, kd);
  return k;
}
__device__ __forceinline__ void kp_stage1_kind(const double* __restrict__ xrow, const double* __restrict__ Z, const double* inv_ell, int Dq, double var,
                                               int kind, int M, int Mp, double* dst, int g, int i16) {
  for (int m0 = g; m0 < Mp; m0 += 16) {
    double r2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < Dq; ++d) {
      const double ie = inv_ell[d], xs = xrow[d] * ie;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = min(m0 + 4 * u, M - 1);      // a point behind M is read as the last one and not used
        const double t = Z[(size_t)m * Dq + d] * ie - xs;
        r2[u] = fma(t, t, r2[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + 4 * u;
      if (m < Mp) dst[m * 16 + i16] = m < M ? kp_value_of_kind(kind, r2[u], var) : 0.0;
    }
  }
}

template <int D, int NST, int RT>
__global__ void __launch_bounds__(256)
k_kron_path_rows(KpArgs pa) {
  extern __shared__ double kp_lds[];
  constexpr int U = 8 / NST;                       // groups of four whose weights are read together: 8 reads of 512 bytes in flight
  const KpLat& a = pa.lat[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, i16 = lane & 15;
  const int waves = blockDim.x >> 6;
  const int64_t row0 = ((int64_t)blockIdx.x * waves + wave) * (RT * 16);
  const int Mt = a.M0 + a.M1p;                     // doubles / 16 of one row tile's region
  double* const region = kp_lds + (size_t)wave * pa.wave_doubles;
  double x[RT][D];
  bool valid[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t n = row0 + t * 16 + i16;
    valid[t] = n < a.N;
#pragma unroll
    for (int d = 0; d < D; ++d) x[t][d] = valid[t] ? a.X[n * D + d] : 0.0;
  }
  // stage 1: the factor values of this wave's rows (a row behind N is read as the first row: finite values, never stored)
  if (row0 < a.N) {
#pragma unroll 1
    for (int t = 0; t < RT; ++t) {
      const int64_t n = row0 + t * 16 + i16;
      const double* xrow = a.X + (n < a.N ? n : 0) * D;
      double* const k0 = region + (size_t)t * Mt * 16;
      kp_stage1(xrow, a.Z0, a.inv_ell, a.D0, a.var0, a.M0, a.M0, k0, g, i16);
      kp_stage1(xrow + a.D0, a.Z1, a.inv_ell + a.D0, a.D1, a.var1, a.M1, a.M1p, k0 + (size_t)a.M0 * 16, g, i16);
    }
  }
  __syncthreads();      // every wave of the block arrives: none has left yet
  if (row0 >= a.N) return;
  const double* const k0s = region + i16;
  const double* const k1s = region + (size_t)a.M0 * 16 + g * 16 + i16;
  const int njg = a.M1p >> 2, ngroups = a.M0 * njg;      // groups of four grid points: group G holds (i, 4 jg + g), G = i njg + jg
  for (int t0 = 0; t0 < pa.ntile; t0 += NST) {
    potrf_d4 acc[RT][NST];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < NST; ++j) acc[t][j] = potrf_d4{0.0, 0.0, 0.0, 0.0};
    // stage 2: the groups in ascending j inside ascending i; the weights of the next U groups are read while these U run (a group
    // behind the last is read as the last and not used)
    if (ngroups > 0) {
      const double* const wp = a.tab + ((int64_t)t0 * a.F + g) * 16 + i16;      // the lane's weight of group G and tile q: wp[(q F + 4 G) 16]
      double cur[U][NST], nxt[U][NST];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < NST; ++q) cur[u][q] = wp[((int64_t)q * a.F + 4 * min(u, ngroups - 1)) * 16];
      int i = 0, jg = 0;
      for (int G0 = 0; G0 < ngroups; G0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < NST; ++q) nxt[u][q] = wp[((int64_t)q * a.F + 4 * min(G0 + U + u, ngroups - 1)) * 16];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (G0 + u < ngroups) {      // wave-uniform
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const double v = __dmul_rn(k0s[((size_t)t * Mt + i) * 16], k1s[((size_t)t * Mt + 4 * jg) * 16]);
#pragma unroll
              for (int q = 0; q < NST; ++q) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[u][q], v, acc[t][q], 0, 0, 0);
            }
            if (++jg == njg) { jg = 0; ++i; }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < NST; ++q) cur[u][q] = nxt[u][q];
      }
    }
    // the cosine loop of k_path_rows, restated (that kernel's code is not touched)
    for (int r = g; r < a.R4; r += 4) {      // R4 is a multiple of 4
      double om[D], wt[NST];
#pragma unroll
      for (int d = 0; d < D; ++d) om[d] = a.omega[(int64_t)r * D + d];
      const double ph = a.phase[r];
#pragma unroll
      for (int q = 0; q < NST; ++q) wt[q] = a.tab[((int64_t)(t0 + q) * a.F + a.coff + r) * 16 + i16];
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        double arg = om[0] * x[t][0];
#pragma unroll
        for (int d = 1; d < D; ++d) arg = fma(om[d], x[t][d], arg);
        const double v = cos(arg + ph);
#pragma unroll
        for (int q = 0; q < NST; ++q) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wt[q], v, acc[t][q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      if (!valid[t]) continue;
      const int64_t n = row0 + t * 16 + i16;
#pragma unroll
      for (int j = 0; j < NST; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int s = (t0 + j) * 16 + 4 * q + g;
          if (s < a.S) a.out[(int64_t)s * a.ldo + n] = acc[t][j][q] + a.shift;
        }
    }
  }
}

// k_kron_path_rows for a launch with a Matern factor on one of its latents: stage 1 is kp_stage1_kind with each factor's kind; stage 2,
// the cosines and the stores -- and with them the one summation order -- are k_kron_path_rows restated.  (One shared body was built
// first: inlined into k_kron_path_rows it changed that kernel's register allocation, and the RBF machine code is to stay what it was;
// profiles/kron_matern_isa.log.)
template <int D, int NST, int RT>
__global__ void __launch_bounds__(256)
k_kron_path_rows_kinds(KpArgs pa) {
  extern __shared__ double kp_lds[];
  constexpr int U = 8 / NST;                       // groups of four whose weights are read together: 8 reads of 512 bytes in flight
  const KpLat& a = pa.lat[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, i16 = lane & 15;
  const int waves = blockDim.x >> 6;
  const int64_t row0 = ((int64_t)blockIdx.x * waves + wave) * (RT * 16);
  const int Mt = a.M0 + a.M1p;                     // doubles / 16 of one row tile's region
  double* const region = kp_lds + (size_t)wave * pa.wave_doubles;
  double x[RT][D];
  bool valid[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t n = row0 + t * 16 + i16;
    valid[t] = n < a.N;
#pragma unroll
    for (int d = 0; d < D; ++d) x[t][d] = valid[t] ? a.X[n * D + d] : 0.0;
  }
  // stage 1: the factor values of this wave's rows (a row behind N is read as the first row: finite values, never stored)
  if (row0 < a.N) {
#pragma unroll 1
    for (int t = 0; t < RT; ++t) {
      const int64_t n = row0 + t * 16 + i16;
      const double* xrow = a.X + (n < a.N ? n : 0) * D;
      double* const k0 = region + (size_t)t * Mt * 16;
      kp_stage1_kind(xrow, a.Z0, a.inv_ell, a.D0, a.var0, a.kinds & 3, a.M0, a.M0, k0, g, i16);
      kp_stage1_kind(xrow + a.D0, a.Z1, a.inv_ell + a.D0, a.D1, a.var1, a.kinds >> 2, a.M1, a.M1p, k0 + (size_t)a.M0 * 16, g, i16);
    }
  }
  __syncthreads();      // every wave of the block arrives: none has left yet
  if (row0 >= a.N) return;
  const double* const k0s = region + i16;
  const double* const k1s = region + (size_t)a.M0 * 16 + g * 16 + i16;
  const int njg = a.M1p >> 2, ngroups = a.M0 * njg;      // groups of four grid points: group G holds (i, 4 jg + g), G = i njg + jg
  for (int t0 = 0; t0 < pa.ntile; t0 += NST) {
    potrf_d4 acc[RT][NST];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < NST; ++j) acc[t][j] = potrf_d4{0.0, 0.0, 0.0, 0.0};
    // stage 2: the groups in ascending j inside ascending i; the weights of the next U groups are read while these U run (a group
    // behind the last is read as the last and not used)
    if (ngroups > 0) {
      const double* const wp = a.tab + ((int64_t)t0 * a.F + g) * 16 + i16;      // the lane's weight of group G and tile q: wp[(q F + 4 G) 16]
      double cur[U][NST], nxt[U][NST];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < NST; ++q) cur[u][q] = wp[((int64_t)q * a.F + 4 * min(u, ngroups - 1)) * 16];
      int i = 0, jg = 0;
      for (int G0 = 0; G0 < ngroups; G0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < NST; ++q) nxt[u][q] = wp[((int64_t)q * a.F + 4 * min(G0 + U + u, ngroups - 1)) * 16];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (G0 + u < ngroups) {      // wave-uniform
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const double v = __dmul_rn(k0s[((size_t)t * Mt + i) * 16], k1s[((size_t)t * Mt + 4 * jg) * 16]);
#pragma unroll
              for (int q = 0; q < NST; ++q) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[u][q], v, acc[t][q], 0, 0, 0);
            }
            if (++jg == njg) { jg = 0; ++i; }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < NST; ++q) cur[u][q] = nxt[u][q];
      }
    }
    // the cosine loop of k_path_rows, restated (that kernel's code is not touched)
    for (int r = g; r < a.R4; r += 4) {      // R4 is a multiple of 4
      double om[D], wt[NST];
#pragma unroll
      for (int d = 0; d < D; ++d) om[d] = a.omega[(int64_t)r * D + d];
      const double ph = a.phase[r];
#pragma unroll
      for (int q = 0; q < NST; ++q) wt[q] = a.tab[((int64_t)(t0 + q) * a.F + a.coff + r) * 16 + i16];
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        double arg = om[0] * x[t][0];
#pragma unroll
        for (int d = 1; d < D; ++d) arg = fma(om[d], x[t][d], arg);
        const double v = cos(arg + ph);
#pragma unroll
        for (int q = 0; q < NST; ++q) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wt[q], v, acc[t][q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      if (!valid[t]) continue;
      const int64_t n = row0 + t * 16 + i16;
#pragma unroll
      for (int j = 0; j < NST; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int s = (t0 + j) * 16 + 4 * q + g;
          if (s < a.S) a.out[(int64_t)s * a.ldo + n] = acc[t][j][q] + a.shift;
        }
    }
  }
}

// ---- the weights of the model calls: S small M0 x M1 problems, one thread per element, k ascending -----------------------------------
// rhs[s][i M1 + j] = U[i][j] + Sq[i][j] E[i M1 + j][s] - FZ[s][i M1 + j]     (E (M, S) as the draw holds it; FZ as the path kernel wrote it)
__global__ void __launch_bounds__(256)
k_kp_rhs(const double* __restrict__ U, const double* __restrict__ Sq, const double* __restrict__ E, const double* __restrict__ FZ, int M, int S,
         double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)M * S) return;
  const int64_t s = idx / M, m = idx - s * M;
  out[idx] = fma(Sq[m], E[m * S + s], U[m]) - FZ[idx];
}

// Y_s = op(A) X_s: A (M0, M0) with row stride lda, op = transpose where ta; X_s, Y_s (M0, M1) at s M0 M1
__global__ void __launch_bounds__(256)
k_kp_left(const double* __restrict__ A, int64_t lda, int ta, const double* __restrict__ X, int M0, int M1, int S, double* __restrict__ Y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t M = (int64_t)M0 * M1;
  if (idx >= M * S) return;
  const int64_t s = idx / M, m = idx - s * M;
  const int i = (int)(m / M1), j = (int)(m - (int64_t)i * M1);
  const double* x = X + s * M + j;
  double v = 0.0;
  for (int k = 0; k < M0; ++k) v = fma(ta ? A[k * lda + i] : A[i * lda + k], x[(int64_t)k * M1], v);
  Y[idx] = v;
}

// Y_s = X_s op(B): B (M1, M1) with row stride ldb, op = transpose where tb
__global__ void __launch_bounds__(256)
k_kp_right(const double* __restrict__ X, const double* __restrict__ B, int64_t ldb, int tb, int M0, int M1, int S, double* __restrict__ Y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t M = (int64_t)M0 * M1;
  if (idx >= M * S) return;
  const int64_t s = idx / M, m = idx - s * M;
  const int i = (int)(m / M1), j = (int)(m - (int64_t)i * M1);
  const double* x = X + s * M + (int64_t)i * M1;
  double v = 0.0;
  for (int k = 0; k < M1; ++k) v = fma(x[k], tb ? B[j * ldb + k] : B[k * ldb + j], v);
  Y[idx] = v;
}

// The grid points' part of a weight table from V[s][i M1 + j]: tab[tile][i M1p + j][c] = V[16 tile + c][i M1 + j] for j < M1 and 16 tile + c < S, else 0
__global__ void __launch_bounds__(256)
k_kp_fill_v(const double* __restrict__ V, int M0, int M1, int M1p, int S, int F, int ntile, double* __restrict__ tab) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t G = (int64_t)M0 * M1p;
  if (idx >= (int64_t)ntile * G * 16) return;
  const int cidx = (int)(idx & 15);
  const int64_t q = idx >> 4;
  const int64_t m = q % G;
  const int tile = (int)(q / G), s = tile * 16 + cidx;
  const int i = (int)(m / M1p), j = (int)(m - (int64_t)i * M1p);
  tab[((int64_t)tile * F + m) * 16 + cidx] = (j < M1 && s < S) ? V[(int64_t)s * M0 * M1 + (int64_t)i * M1 + j] : 0.0;
}

// out[idx] = dn_link(f[idx]): the Bernoulli head's probability plane
__global__ void __launch_bounds__(256)
k_kp_probit(const double* __restrict__ f, double* __restrict__ out, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < n) out[idx] = dn_link(f[idx]);
}

}  // namespace zigp

namespace {

// Sample tiles per pass: as path_tiles_per_pass (env ZIGP_PATH_TILES = 1, 2 or 4 caps it); the choice moves no bit of the result.
struct KpDims { int M1p, R4, F, coff; };
KpDims kp_dims(int M0, int M1, int R) {
  KpDims d;
  d.M1p = (int)round_up(M1, 4); d.R4 = (int)round_up(std::max(R, 0), 4); d.coff = M0 * d.M1p; d.F = d.coff + d.R4;
  return d;
}

template <int D, int RT>
int kp_launch_rt(zigp_ctx* c, const KpArgs& pa, int nlat, int nst, int64_t maxN, int waves) {
  const dim3 grid((unsigned)ceil_div(maxN, (int64_t)waves * RT * 16), (unsigned)nlat), block(64 * waves);
  const size_t shm = sizeof(double) * (size_t)pa.wave_doubles * waves;
  bool kinds = false;      // a Matern factor on a latent of this launch: the instantiations with the kind switch in stage 1
  for (int h = 0; h < nlat; ++h) kinds = kinds || pa.lat[h].kinds != 0;
  if (kinds) {
    if (nst == 4) hipLaunchKernelGGL((k_kron_path_rows_kinds<D, 4, RT>), grid, block, shm, c->stream, pa);
    else if (nst == 2) hipLaunchKernelGGL((k_kron_path_rows_kinds<D, 2, RT>), grid, block, shm, c->stream, pa);
    else hipLaunchKernelGGL((k_kron_path_rows_kinds<D, 1, RT>), grid, block, shm, c->stream, pa);
  } else if (nst == 4) hipLaunchKernelGGL((k_kron_path_rows<D, 4, RT>), grid, block, shm, c->stream, pa);
  else if (nst == 2) hipLaunchKernelGGL((k_kron_path_rows<D, 2, RT>), grid, block, shm, c->stream, pa);
  else hipLaunchKernelGGL((k_kron_path_rows<D, 1, RT>), grid, block, shm, c->stream, pa);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
template <int D>
int kp_launch_d(zigp_ctx* c, const KpArgs& pa, int nlat, int nst, int64_t maxN, int waves, int rt) {
  return rt == 2 ? kp_launch_rt<D, 2>(c, pa, nlat, nst, maxN, waves) : kp_launch_rt<D, 1>(c, pa, nlat, nst, maxN, waves);
}
// The row tiles of a wave, its LDS region and the waves of a block follow from the latents' grids (M0 = M1p = 0: the cosines alone).
// Two row tiles a wave share every weight read; they are taken where four such waves fit a block's LDS (M0 + M1p <= 64: two blocks a CU,
// two waves per SIMD), else one tile a wave.  The choice moves no bit of the result.
int kp_launch(zigp_ctx* c, int D, KpArgs& pa, int nlat, int nst) {
  int64_t maxN = 0;
  int mt = 0;
  for (int h = 0; h < nlat; ++h) { maxN = std::max(maxN, pa.lat[h].N); mt = std::max(mt, pa.lat[h].M0 + pa.lat[h].M1p); }
  if (maxN <= 0) return 0;
  const int rt = (size_t)KP_RT * mt * 16 * sizeof(double) * 4 <= (size_t)KP_LDS_BYTES ? KP_RT : 1;
  pa.wave_doubles = rt * mt * 16;
  const size_t wave_bytes = sizeof(double) * (size_t)pa.wave_doubles;
  if (wave_bytes > (size_t)KP_LDS_BYTES) return fail_arg(c, "the Kronecker path kernel covers M0 + M1 <= 256");
  const int waves = wave_bytes * 4 <= (size_t)KP_LDS_BYTES ? 4 : wave_bytes * 2 <= (size_t)KP_LDS_BYTES ? 2 : 1;
  switch (D) {
    case 2: return kp_launch_d<2>(c, pa, nlat, nst, maxN, waves, rt);
    case 3: return kp_launch_d<3>(c, pa, nlat, nst, maxN, waves, rt);
    case 4: return kp_launch_d<4>(c, pa, nlat, nst, maxN, waves, rt);
    case 5: return kp_launch_d<5>(c, pa, nlat, nst, maxN, waves, rt);
    case 6: return kp_launch_d<6>(c, pa, nlat, nst, maxN, waves, rt);
    case 7: return kp_launch_d<7>(c, pa, nlat, nst, maxN, waves, rt);
    case 8: return kp_launch_d<8>(c, pa, nlat, nst, maxN, waves, rt);
    default: return fail_arg(c, "the Kronecker path kernel covers D0 + D1 in [2, 8]");
  }
}

int kp_check_dims(zigp_ctx* c, const std::string& w, int D0, int D1, int S, int64_t N) {
  if (D0 < 1 || D1 < 1) return refuse(c, w, "D0 = " + std::to_string(D0) + ", D1 = " + std::to_string(D1) + ": D0 and D1 must be positive");
  if (D0 + D1 > MAXD)
    return refuse(c, w, "D0 + D1 = " + std::to_string(D0 + D1) + ": the Kronecker path kernel covers D0 + D1 <= 8");
  if (S < 1 || S > PT_MAXS) return refuse(c, w, "S = " + std::to_string(S) + " must be in [1, 256] (ZIGP_PATH_MAX_S)");
  if (N < 0) return refuse(c, w, "N is negative");
  return 0;
}
int kp_check_grid(zigp_ctx* c, const std::string& w, int M0, int M1) {
  if (M0 < 1 || M0 > KP_MAXM) return refuse(c, w, "M0 = " + std::to_string(M0) + " must be in [1, 128]");
  if (M1 < 1 || M1 > KP_MAXM) return refuse(c, w, "M1 = " + std::to_string(M1) + " must be in [1, 128]");
  return 0;
}
void kp_inv_ell(KpLat& a, const double* ell0, const double* ell1, int D0, int D1) {
  for (int d = 0; d < MAXD; ++d) a.inv_ell[d] = d < D0 ? 1.0 / ell0[d] : d < D0 + D1 ? 1.0 / ell1[d - D0] : 0.0;
}

// zigp_kron_path_rows and zigp_kron_path_rows_device
int kron_path_rows(zigp_ctx* c, const char* who, const zigp_kron_path_latent* lat, int nlat, int D0, int D1, int S, const double* X, int64_t N,
                   double* out, bool on_device) {
  if (!c) return ZIGP_EARG;
  const std::string w(who);
  if (!lat) return refuse(c, w, "lat is NULL");
  if (nlat != 1 && nlat != 2) return refuse(c, w, "nlat must be 1 or 2");
  ZIGP_TRY(kp_check_dims(c, w, D0, D1, S, N));
  const int D = D0 + D1;
  for (int h = 0; h < nlat; ++h) {
    const zigp_kron_path_latent& q = lat[h];
    ZIGP_TRY(kp_check_grid(c, w, q.M0, q.M1));
    if (q.R < 0) return refuse(c, w, "R is negative");
    if (q.reserved < 0 || q.reserved > 10 || (q.reserved & 3) == 3)      // the record's `reserved` word carries the kinds
      return refuse(c, w, "kinds = " + std::to_string(q.reserved) + " is not kind0 + 4 kind1 of two ZIGP_KERN_* values");
    ZIGP_TRY(path_check_table(c, w, "Z0", q.Z0, (size_t)q.M0 * D0));
    ZIGP_TRY(path_check_table(c, w, "Z1", q.Z1, (size_t)q.M1 * D1));
    ZIGP_TRY(path_check_table(c, w, "ell0", q.ell0, D0));
    ZIGP_TRY(path_check_table(c, w, "ell1", q.ell1, D1));
    ZIGP_TRY(path_check_table(c, w, "V", q.V, (size_t)q.M0 * q.M1 * S));
    ZIGP_TRY(path_check_table(c, w, "omega", q.omega, (size_t)q.R * D));
    ZIGP_TRY(path_check_table(c, w, "phase", q.phase, q.R));
    ZIGP_TRY(path_check_table(c, w, "amp", q.amp, (size_t)q.R * S));
    if (!std::isfinite(q.shift)) return refuse(c, w, "shift is not finite");
    if (!(q.var0 > 0 && std::isfinite(q.var0))) return refuse(c, w, "var0 must be positive and finite");
    if (!(q.var1 > 0 && std::isfinite(q.var1))) return refuse(c, w, "var1 must be positive and finite");
    for (int d = 0; d < D0; ++d)
      if (!(q.ell0[d] > 0)) return refuse(c, w, "ell0 must be positive");
    for (int d = 0; d < D1; ++d)
      if (!(q.ell1[d] > 0)) return refuse(c, w, "ell1 must be positive");
  }
  if (N > 0 && (!X || !out)) return refuse(c, w, "X or out is NULL");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device) ZIGP_TRY(require_device_ptrs(c, {X, out}, (w + ": X and out must be device memory of the context's GPU").c_str()));
  ZIGP_TRY(begin_staged_call(c));
  const int nst = path_tiles_per_pass(S), ntile = (int)round_up((S + 15) / 16, nst);
  // one staged image: per latent [Z0 | Z1 | omega | phase | table]
  size_t off[2][5], total = 0;
  KpDims dm[2];
  for (int h = 0; h < nlat; ++h) {
    dm[h] = kp_dims(lat[h].M0, lat[h].M1, lat[h].R);
    off[h][0] = total; total += (size_t)lat[h].M0 * D0;
    off[h][1] = total; total += (size_t)lat[h].M1 * D1;
    off[h][2] = total; total += (size_t)dm[h].R4 * D;
    off[h][3] = total; total += (size_t)dm[h].R4;
    off[h][4] = total; total += (size_t)ntile * dm[h].F * 16;
  }
  ZIGP_ENSURE(c, c->path_tab, total);
  ZIGP_PINNED(c, img, total);
  memset(img, 0, sizeof(double) * total);
  KpArgs pa{};
  pa.ntile = ntile;
  for (int h = 0; h < nlat; ++h) {
    const zigp_kron_path_latent& q = lat[h];
    memcpy(img + off[h][0], q.Z0, sizeof(double) * q.M0 * D0);
    memcpy(img + off[h][1], q.Z1, sizeof(double) * q.M1 * D1);
    if (q.R > 0) {
      memcpy(img + off[h][2], q.omega, sizeof(double) * q.R * D);
      memcpy(img + off[h][3], q.phase, sizeof(double) * q.R);
    }
    double* tab = img + off[h][4];
    for (int s = 0; s < S; ++s) {
      double* tt = tab + (size_t)(s >> 4) * dm[h].F * 16 + (s & 15);
      for (int i = 0; i < q.M0; ++i)
        for (int j = 0; j < q.M1; ++j) tt[((size_t)i * dm[h].M1p + j) * 16] = q.V[((size_t)i * q.M1 + j) * S + s];
      for (int r = 0; r < q.R; ++r) tt[(size_t)(dm[h].coff + r) * 16] = q.amp[(size_t)r * S + s];
    }
    KpLat& a = pa.lat[h];
    const double* base = c->path_tab.p;
    a.N = N; a.Z0 = base + off[h][0]; a.Z1 = base + off[h][1]; a.omega = base + off[h][2]; a.phase = base + off[h][3]; a.tab = base + off[h][4];
    a.ldo = N; a.M0 = q.M0; a.M1 = q.M1; a.M1p = dm[h].M1p; a.R4 = dm[h].R4; a.F = dm[h].F; a.coff = dm[h].coff; a.S = S; a.D0 = D0; a.D1 = D1;
    kp_inv_ell(a, q.ell0, q.ell1, D0, D1);
    a.var0 = q.var0; a.var1 = q.var1; a.shift = q.shift;
    a.kinds = q.reserved;
  }
  ZIGP_HIP(c, hipMemcpyAsync(c->path_tab.p, img, sizeof(double) * total, hipMemcpyHostToDevice, c->stream));
  const double* dX = nullptr;
  ZIGP_TRY(stage_inputs(c, X, N, D, on_device, &dX));
  if (!on_device) ZIGP_ENSURE(c, c->path_out, (size_t)nlat * S * N);
  double* dout = on_device ? out : c->path_out.p;
  for (int h = 0; h < nlat; ++h) { pa.lat[h].X = dX; pa.lat[h].out = dout + (size_t)h * S * N; }
  ZIGP_TRY(kp_launch(c, D, pa, nlat, nst));
  return finish_copies(c, {{on_device ? nullptr : out, dout, (size_t)nlat * S * N}});
}

// One step of iterative refinement of the weights, V += K0^-1 (rhs - K0 V K1) K1^-1, was built and measured, and is not part of the
// product build: on the model fixtures (tools/kron_paths_parity.py, profiles/kron_paths_parity.log) a path is 7e-14 .. 3e-11 from the
// restatement with the step and 3e-15 .. 2e-11 without it, under bounds of 2e-9 .. 1e-6 -- equally far inside.  Unlike the dense weights,
// whose W^T W of one M x M factor of cond 4e8 needed the step, each W_p here belongs to one factor.  A build with
// -DZIGP_KRON_PATH_REFINE (tools/build_variant.sh) compiles the step in, for that tool alone.  The claim is held by a test: the residual
// rhs_s - K0 V_s K1 of the unrefined weights is within 4 res_np + 16 eps (|K0| |V_s| |K1| + |rhs_s|) per element on the model fixtures and the
// 32 x 32 precipitation init (tests/test_gpu_path_weight_stages.py through zigp_test_kron_path_weights; measured <= 3.8 eps S_w).

int kp_elementwise_grid(int64_t n) { return (int)ceil_div(n, (int64_t)256); }

struct KronPathTap : PathTap { const zigp_stage_kron_path_weights* s; int64_t facts[ZIGP_KWF_COUNT]; };
// KW_SNAP(field, device pointer, count): latent h's tap of that name (zigp_test_kron_path_weights); a no-op without a sink
#define KW_SNAP(field, dev, n) do { if (tap) ZIGP_TRY(tap->snap(c, tap->s->lat[h].field, (dev), (n))); } while (0)

// The weight stage of the Kronecker model calls behind the call's own factor forward stage: the device tables of the latents, f_Z by the
// path kernel at the grid points, V_s = W0^T (W0 rhs_s W1^T) W1 and the grid points' part of the weight table.  pa comes back as the
// argument record of the path launch at Xnew (X, N, out, ldo and shift are the caller's to set).
int kron_path_weight_stage(zigp_ctx* c, KronState& ks, const KronHostLatent (&hl)[2], int nlat, const zigp_path_draw* const (&dr)[2], int D0, int D1,
                           int S, int nst, KpArgs& pa, KronPathTap* tap) {
  const int D = D0 + D1, ntile = (int)round_up((S + 15) / 16, nst);
  // device tables per latent: [omega | phase | table | E | U | Sq | grid rows] staged from the host, then [FZ | R | A | B | V] work matrices (S, M)
  size_t off[2][12], total = 0, staged = 0;
  KpDims dm[2];
  for (int h = 0; h < nlat; ++h) {
    const size_t M = (size_t)hl[h].M[0] * hl[h].M[1];
    dm[h] = kp_dims(hl[h].M[0], hl[h].M[1], dr[h]->R);
    off[h][0] = total; total += (size_t)dm[h].R4 * D;
    off[h][1] = total; total += (size_t)dm[h].R4;
    off[h][2] = total; total += (size_t)ntile * dm[h].F * 16;
    off[h][3] = total; total += M * S;       // E (M, S)
    off[h][4] = total; total += M;           // U
    off[h][5] = total; total += M;           // Sq
    off[h][6] = total; total += M * D;       // the grid points as rows (M, D)
  }
  staged = total;
  for (int h = 0; h < nlat; ++h) {
    const size_t M = (size_t)hl[h].M[0] * hl[h].M[1];
    for (int k = 7; k < 12; ++k) { off[h][k] = total; total += M * S; }      // FZ, R, A, B, V
  }
  ZIGP_ENSURE(c, c->path_tab, total);
  double* base = c->path_tab.p;
  ZIGP_PINNED(c, img, staged);
  memset(img, 0, sizeof(double) * staged);
  pa = KpArgs{};
  pa.ntile = ntile;
  for (int h = 0; h < nlat; ++h) {
    const int R = dr[h]->R, M0 = hl[h].M[0], M1 = hl[h].M[1];
    const size_t M = (size_t)M0 * M1;
    for (int r = 0; r < R; ++r) {
      for (int d = 0; d < D; ++d)
        img[off[h][0] + (size_t)r * D + d] = dr[h]->omega0[(size_t)r * D + d] / (d < D0 ? hl[h].ell[0][d] : hl[h].ell[1][d - D0]);
      img[off[h][1] + r] = dr[h]->phase[r];
    }
    const double knn = hl[h].var[0] * hl[h].var[1];
    const double ampl = R > 0 ? sqrt(2.0 * knn / R) : 0.0;
    double* tab = img + off[h][2];
    for (int s = 0; s < S; ++s) {
      double* tt = tab + (size_t)(s >> 4) * dm[h].F * 16 + (s & 15);
      for (int r = 0; r < R; ++r) tt[(size_t)(dm[h].coff + r) * 16] = dr[h]->a[(size_t)r * S + s] * ampl;
    }
    memcpy(img + off[h][3], dr[h]->eps, sizeof(double) * M * S);
    memcpy(img + off[h][4], hl[h].u, sizeof(double) * M);
    memcpy(img + off[h][5], hl[h].s, sizeof(double) * M);
    double* G = img + off[h][6];
    for (int i = 0; i < M0; ++i)
      for (int j = 0; j < M1; ++j) {
        double* row = G + ((size_t)i * M1 + j) * D;
        for (int d = 0; d < D0; ++d) row[d] = hl[h].Z[0][(size_t)i * D0 + d];
        for (int d = 0; d < D1; ++d) row[D0 + d] = hl[h].Z[1][(size_t)j * D1 + d];
      }
    KpLat& a = pa.lat[h];
    a.Z0 = ks.lat[h].f[0].Z.p; a.Z1 = ks.lat[h].f[1].Z.p; a.omega = base + off[h][0]; a.phase = base + off[h][1]; a.tab = base + off[h][2];
    a.M0 = M0; a.M1 = M1; a.M1p = dm[h].M1p; a.R4 = dm[h].R4; a.F = dm[h].F; a.coff = dm[h].coff; a.S = S; a.D0 = D0; a.D1 = D1;
    kp_inv_ell(a, hl[h].ell[0], hl[h].ell[1], D0, D1);
    a.var0 = hl[h].var[0]; a.var1 = hl[h].var[1]; a.shift = 0.0;
    a.kinds = hl[h].kind[0] + 4 * hl[h].kind[1];
  }
  ZIGP_HIP(c, hipMemcpyAsync(base, img, sizeof(double) * staged, hipMemcpyHostToDevice, c->stream));
  if (tap) {      // the hook: every work matrix (S, M) is written completely by its launch
    tap->facts[ZIGP_KWF_NST] = nst; tap->facts[ZIGP_KWF_NTILE] = ntile;
    ZIGP_TRY(tap->sentinel(c, base + staged, total - staged));
    for (int h = 0; h < nlat; ++h) {
      const size_t M = (size_t)hl[h].M[0] * hl[h].M[1];
      tap->facts[ZIGP_KWF_M1P + h] = dm[h].M1p; tap->facts[ZIGP_KWF_R4 + h] = dm[h].R4; tap->facts[ZIGP_KWF_F + h] = dm[h].F;
      for (int q = 0; q < 2; ++q) {
        const KronFactor& f = ks.lat[h].f[q];
        tap->facts[(q ? ZIGP_KWF_MQ1 : ZIGP_KWF_MQ0) + h] = f.Mq;
        KW_SNAP(K[q], f.K.p, (size_t)f.Mq * f.Mq); KW_SNAP(W[q], f.W.p, (size_t)f.Mq * f.Mq);
      }
      KW_SNAP(E, base + off[h][3], M * S); KW_SNAP(U, base + off[h][4], M); KW_SNAP(Sq, base + off[h][5], M);
    }
  }

  // f_Z: the cosines alone at the grid points (no grid group runs), written as (S, M)
  KpArgs pz = pa;
  for (int h = 0; h < nlat; ++h) {
    KpLat& a = pz.lat[h];
    a.X = base + off[h][6]; a.N = (int64_t)hl[h].M[0] * hl[h].M[1]; a.M0 = 0; a.M1 = 0; a.M1p = 0; a.out = base + off[h][7]; a.ldo = a.N;
  }
  ZIGP_TRY(kp_launch(c, D, pz, nlat, nst));

  // V_s = W0^T (W0 rhs_s W1^T) W1
  for (int h = 0; h < nlat; ++h) {
    const int M0 = hl[h].M[0], M1 = hl[h].M[1], M = M0 * M1;
    const KronFactor &f0 = ks.lat[h].f[0], &f1 = ks.lat[h].f[1];
    double *E = base + off[h][3], *U = base + off[h][4], *Sq = base + off[h][5];
    double *FZ = base + off[h][7], *Rh = base + off[h][8], *A = base + off[h][9], *B = base + off[h][10], *V = base + off[h][11];
    const int64_t n = (int64_t)M * S;
    const dim3 grid((unsigned)kp_elementwise_grid(n)), block(256);
    // dst = K0^-1 src K1^-1 through the explicit W_p: (W0^T (W0 src W1^T)) W1; A and B are the work matrices
    auto solve = [&](const double* src, double* dst, bool taps) -> int {
      hipLaunchKernelGGL(k_kp_left, grid, block, 0, c->stream, f0.W.p, (int64_t)f0.Mq, 0, src, M0, M1, S, A);       // W0 src
      if (taps) KW_SNAP(A1, A, (size_t)n);
      hipLaunchKernelGGL(k_kp_right, grid, block, 0, c->stream, A, f1.W.p, (int64_t)f1.Mq, 1, M0, M1, S, B);        // .. W1^T
      if (taps) KW_SNAP(B1, B, (size_t)n);
      hipLaunchKernelGGL(k_kp_left, grid, block, 0, c->stream, f0.W.p, (int64_t)f0.Mq, 1, B, M0, M1, S, A);         // W0^T ..
      if (taps) KW_SNAP(A2, A, (size_t)n);
      hipLaunchKernelGGL(k_kp_right, grid, block, 0, c->stream, A, f1.W.p, (int64_t)f1.Mq, 0, M0, M1, S, dst);      // .. W1
      return 0;
    };
    KW_SNAP(FZ, FZ, (size_t)n);
    hipLaunchKernelGGL(k_kp_rhs, grid, block, 0, c->stream, U, Sq, E, FZ, M, S, Rh);
    KW_SNAP(rhs, Rh, (size_t)n);
    ZIGP_TRY(solve(Rh, V, true));
#ifdef ZIGP_KRON_PATH_REFINE
    {
      // What reaches a path is the residual of V (zigp_paths.hip, the dense refinement): V += K0^-1 (rhs - K0 V K1) K1^-1.  K_p is
      // factor_forward's matrix, jitter included; f_Z has no reader left, its buffer takes the residual and then the correction.
      hipLaunchKernelGGL(k_kp_left, grid, block, 0, c->stream, f0.K.p, (int64_t)f0.Mq, 0, V, M0, M1, S, A);         // K0 V
      hipLaunchKernelGGL(k_kp_right, grid, block, 0, c->stream, A, f1.K.p, (int64_t)f1.Mq, 0, M0, M1, S, B);        // .. K1
      hipLaunchKernelGGL(k_path_axpy, grid, block, 0, c->stream, Rh, -1.0, B, n, FZ);                                // residual
      ZIGP_TRY(solve(FZ, FZ, false));
      hipLaunchKernelGGL(k_path_axpy, grid, block, 0, c->stream, V, 1.0, FZ, n, V);
    }
#endif
    KW_SNAP(V, V, (size_t)n);
    if (tap)      // k_kp_fill_v writes every grid row of the table
      for (int tile = 0; tile < ntile; ++tile) ZIGP_TRY(tap->sentinel(c, base + off[h][2] + (size_t)tile * dm[h].F * 16, (size_t)dm[h].coff * 16));
    const int64_t nfill = (int64_t)ntile * dm[h].coff * 16;
    hipLaunchKernelGGL(k_kp_fill_v, dim3((unsigned)kp_elementwise_grid(nfill)), block, 0, c->stream, V, M0, M1, dm[h].M1p, S, dm[h].F, ntile,
                       base + off[h][2]);
    ZIGP_HIP(c, hipGetLastError());
    KW_SNAP(tab, base + off[h][2], (size_t)ntile * dm[h].F * 16);
  }
  return 0;
}

// zigp_kron_sample_paths[_device] (lik = ZIGP_LIK_ONOFF: out (3, S, N)) and zigp_kron_head_sample_paths[_device] (out (1 or 2, S, N))
int kron_sample_paths(zigp_ctx* c, const char* who, const zigp_kron_params* p, int lik, const double* X, int64_t N, double jitter, double g_offset,
                      double f_mu, const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int S, double* out, bool on_device,
                      KronPathTap* tap = nullptr) {      // tap: zigp_test_kron_path_weights -- the weight stage alone, no rows
  if (!c) return ZIGP_EARG;
  const std::string w(who);
  if (lik != ZIGP_LIK_ONOFF && lik != ZIGP_LIK_GAUSSIAN && lik != ZIGP_LIK_BERNOULLI)
    return refuse(c, w, "lik must be ZIGP_LIK_GAUSSIAN or ZIGP_LIK_BERNOULLI");
  if (p) ZIGP_TRY(kp_check_dims(c, w, p->D0, p->D1, S, N));      // names D0 + D1 before validate_kron speaks of the factor dimensions
  ZIGP_TRY(validate_kron(c, p, lik));
  const int nlat = lik == ZIGP_LIK_ONOFF ? 2 : 1, D0 = p->D0, D1 = p->D1, D = D0 + D1;
  KronHostLatent hl[2];
  kron_host_latents(p, nlat, hl);
  kron_set_kinds(c, hl, nlat);      // zigp_set_kron_kernel: the factor stage and the path kernel evaluate the same k_q
  const zigp_path_draw* dr[2] = {draw_f, draw_g};
  const char* tag[2] = {"f", "g"};
  for (int h = 0; h < nlat; ++h) {
    ZIGP_TRY(kp_check_grid(c, w, hl[h].M[0], hl[h].M[1]));
    ZIGP_TRY(path_check_draw(c, w, tag[h], dr[h], hl[h].M[0] * hl[h].M[1], D, S));
    const size_t M = (size_t)hl[h].M[0] * hl[h].M[1];
    ZIGP_TRY(path_check_table(c, w, h ? "u_gm" : "u_fm", hl[h].u, M));
    ZIGP_TRY(path_check_table(c, w, h ? "u_gs_sqrt" : "u_fs_sqrt", hl[h].s, M));
    for (int q = 0; q < 2; ++q) {
      const int Dq = q ? D1 : D0;
      ZIGP_TRY(path_check_table(c, w, q ? "Z1" : "Z0", hl[h].Z[q], (size_t)hl[h].M[q] * Dq));
      ZIGP_TRY(path_check_table(c, w, q ? "ell1" : "ell0", hl[h].ell[q], Dq));
      for (int d = 0; d < Dq; ++d)
        if (!(hl[h].ell[q][d] > 0)) return refuse(c, w, "lengthscales must be positive");
      if (!std::isfinite(hl[h].var[q])) return refuse(c, w, "variances must be finite");
    }
  }
  if (!(jitter >= 0)) return refuse(c, w, "jitter must be >= 0");
  if (!std::isfinite(g_offset)) return refuse(c, w, "g_offset is not finite");
  if (!std::isfinite(f_mu)) return refuse(c, w, "f_mu is not finite");
  if (!tap && N > 0 && (!X || !out)) return refuse(c, w, "Xnew or out is NULL");
  if (!tap && N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device) ZIGP_TRY(require_device_ptrs(c, {X, out}, (w + ": Xnew and out must be device memory of the context's GPU").c_str()));
  if (!c->kron) { c->kron.reset(new (std::nothrow) KronState()); if (!c->kron) { c->err = "out of memory"; return ZIGP_EHIP; } }
  KronState& ks = *c->kron;
  ZIGP_TRY(begin_staged_call(c));

  // the call's own factor forward stage, as zigp_kron_predict's panel path runs it: K_p + jitter I, L_p, W_p = L_p^-1
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  for (int h = 0; h < nlat; ++h) {
    ZIGP_TRY(factor_forward(c, ks.lat[h].f[0], hl[h].M[0], D0, 0, hl[h].Z[0], hl[h].ell[0], hl[h].var[0], jitter, hl[h].kind[0]));
    ZIGP_TRY(factor_forward(c, ks.lat[h].f[1], hl[h].M[1], D1, D0, hl[h].Z[1], hl[h].ell[1], hl[h].var[1], jitter, hl[h].kind[1]));
  }
  int* hinfo = nullptr;
  ZIGP_TRY(request_info(c, &hinfo));

  const int nst = path_tiles_per_pass(S);
  KpArgs pa{};
  ZIGP_TRY(kron_path_weight_stage(c, ks, hl, nlat, dr, D0, D1, S, nst, pa, tap));
  if (tap) {
    ZIGP_TRY(finish_copies(c, {}));
    ZIGP_TRY(tap->flush(c));
    return info_result(c, hinfo, kron_fac_any);
  }

  // the paths at Xnew: f_mu on f, g_offset on g
  const double* dX = nullptr;
  ZIGP_TRY(stage_inputs(c, X, N, D, on_device, &dX));
  const int planes = lik == ZIGP_LIK_ONOFF ? 3 : lik == ZIGP_LIK_BERNOULLI ? 2 : 1;
  const int64_t SN = (int64_t)S * N;
  if (!on_device) ZIGP_ENSURE(c, c->path_out, (size_t)planes * SN);
  double* dout = on_device ? out : c->path_out.p;
  for (int h = 0; h < nlat; ++h) {
    KpLat& a = pa.lat[h];
    a.X = dX; a.N = N; a.out = dout + (size_t)h * SN; a.ldo = N;
  }
  pa.lat[0].shift = f_mu;
  if (nlat == 2) pa.lat[1].shift = g_offset;
  ZIGP_TRY(kp_launch(c, D, pa, nlat, nst));
  const dim3 egrid((unsigned)kp_elementwise_grid(SN));
  if (lik == ZIGP_LIK_ONOFF) hipLaunchKernelGGL(k_path_gf, egrid, dim3(256), 0, c->stream, dout, dout + SN, dout + 2 * SN, SN);
  else if (lik == ZIGP_LIK_BERNOULLI) hipLaunchKernelGGL(k_kp_probit, egrid, dim3(256), 0, c->stream, dout, dout + SN, SN);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(finish_copies(c, {{on_device ? nullptr : out, dout, (size_t)planes * SN}}));
  return info_result(c, hinfo, kron_fac_any);
}

}  // namespace

extern "C" {

int zigp_kron_path_rows(zigp_ctx* c, const zigp_kron_path_latent* lat, int32_t nlat, int32_t D0, int32_t D1, int32_t S, const double* X, int64_t N,
                        double* out) {
  return kron_path_rows(c, "zigp_kron_path_rows", lat, nlat, D0, D1, S, X, N, out, false);
}

int zigp_kron_path_rows_device(zigp_ctx* c, const zigp_kron_path_latent* lat, int32_t nlat, int32_t D0, int32_t D1, int32_t S, const double* dX,
                               int64_t N, double* d_out) {
  return kron_path_rows(c, "zigp_kron_path_rows_device", lat, nlat, D0, D1, S, dX, N, d_out, true);
}

int zigp_kron_sample_paths(zigp_ctx* c, const zigp_kron_params* p, const double* Xnew, int64_t N, double jitter, double g_offset, double f_mu,
                           const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* out3) {
  return kron_sample_paths(c, "zigp_kron_sample_paths", p, ZIGP_LIK_ONOFF, Xnew, N, jitter, g_offset, f_mu, draw_f, draw_g, S, out3, false);
}

int zigp_kron_sample_paths_device(zigp_ctx* c, const zigp_kron_params* p, const double* dXnew, int64_t N, double jitter, double g_offset,
                                  double f_mu, const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* d_out3) {
  return kron_sample_paths(c, "zigp_kron_sample_paths_device", p, ZIGP_LIK_ONOFF, dXnew, N, jitter, g_offset, f_mu, draw_f, draw_g, S, d_out3, true);
}

int zigp_kron_head_sample_paths(zigp_ctx* c, const zigp_kron_params* p, int32_t lik, const double* Xnew, int64_t N, double jitter, double f_mu,
                                const zigp_path_draw* draw_f, int32_t S, double* out) {
  if (c && lik == ZIGP_LIK_ONOFF) return refuse(c, "zigp_kron_head_sample_paths", "use zigp_kron_sample_paths for the OnOff likelihood");
  return kron_sample_paths(c, "zigp_kron_head_sample_paths", p, lik, Xnew, N, jitter, 0.0, f_mu, draw_f, nullptr, S, out, false);
}

int zigp_kron_head_sample_paths_device(zigp_ctx* c, const zigp_kron_params* p, int32_t lik, const double* dXnew, int64_t N, double jitter,
                                       double f_mu, const zigp_path_draw* draw_f, int32_t S, double* d_out) {
  if (c && lik == ZIGP_LIK_ONOFF) return refuse(c, "zigp_kron_head_sample_paths_device", "use zigp_kron_sample_paths_device for the OnOff likelihood");
  return kron_sample_paths(c, "zigp_kron_head_sample_paths_device", p, lik, dXnew, N, jitter, 0.0, f_mu, draw_f, nullptr, S, d_out, true);
}

// The weight stage of zigp_kron_sample_paths / zigp_kron_head_sample_paths through kron_sample_paths itself -- its checks, its factor
// forward stage, kron_path_weight_stage -- with the device buffers snapshot (KronPathTap); the paths at Xnew are not run.
int zigp_test_kron_path_weights(zigp_ctx* c, const zigp_stage_kron_path_weights* s) {
  if (!c) return ZIGP_EARG;
  if (!s) return refuse(c, "zigp_test_kron_path_weights", "the record is NULL");
  KronPathTap tap;
  tap.s = s;
  memset(tap.facts, 0, sizeof(tap.facts));
  ZIGP_TRY(kron_sample_paths(c, "zigp_test_kron_path_weights", s->p, s->lik, nullptr, 0, s->jitter, 0.0, 0.0, s->draw_f,
                             s->lik == ZIGP_LIK_ONOFF ? s->draw_g : nullptr, s->S, nullptr, false, &tap));
  if (s->facts) memcpy(s->facts, tap.facts, sizeof(tap.facts));
  return ZIGP_OK;
}

}  // extern "C"
