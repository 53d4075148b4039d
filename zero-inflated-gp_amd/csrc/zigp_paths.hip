// Posterior sample paths at test inputs by decoupled pathwise conditioning (include/zigp.h "sample paths").
//
// Per latent h, test row n and sample s this finite sum is the definition (zigp_path_rows computes it and nothing else):
//   out[h][s][n] = shift_h + sum_d lin_h[d] x[n][d]
//                + sum_{m < M} V_h[m][s] k_h(x_n, z_m)
//                + sum_{r < R} amp_h[r][s] cos( sum_d omega_h[r][d] x[n][d] + phase_h[r] )
// k_h is the Kuf panel's element function: inputs scaled by KUF_C / ell_d, w = -sum_d (zs_d - xs_d)^2 in ascending d, then kuf_exp2_32
// (RBF) or kuf_matern (kuf_sqrt, the floored distance) of zigp_kernels.h, as they are -- a path and a panel agree on what k is.
//
// k_path_rows<D, NST>: a 16 x (M + R) by (M + R) x rows product per tile of 16 samples whose B operand is generated in registers.
//   block = 4 waves, a wave owns PT_RT = 2 tiles of 16 rows (its rows' x in registers, raw and scaled); grid (ceil(N / 128), latents):
//   both latents in one launch, the kernel kind is uniform over a block.
//   A (weights) : A[sample = l & 15][k = l >> 4], one coalesced 512-byte read per group of four features and sample tile from the
//                 [sample tile][feature][16] table (kernel features first, then cosines; M and R padded to multiples of 4 and S to
//                 16 with ZERO weights, so a group never mixes a kernel value with a cosine and the branch is wave-uniform)
//   B (features): B[k = l >> 4][row = l & 15], lane l computes ONE feature of ONE row per instruction
//   D           : v_mfma_f64_16x16x4_f64, c[r] of lane l = D[sample 4 r + (l >> 4)][row l & 15], stored as 128-byte runs of out[s][n ...]
//   A pass carries NST sample tiles (1, 2 or 4): a feature value is computed once and used for 16 NST samples.
// One summation order per element: the accumulator starts at +0, takes the groups of four kernel features in ascending m, then the
// groups of four cosines in ascending r (the order inside a group is the instruction's), and the mean part shift + sum_d lin_d x_d
// (fused multiply-adds, ascending d) is added last.  A padded feature adds an exact 0 * finite.  Nothing depends on N, on the row's
// position, on S, on the sample's column, on NST or on the other latent: the same bits for the same row, sample and tables.
// The cosine is the device library's cos (full-range argument reduction): correct for every finite argument, the arguments beyond
// its fast range (about 1e5 .. 1e6 and up) take its slower reduction path.  Non-finite table entries are refused on the host.
//
// Resources on gfx950 (-Rpass-analysis=kernel-resource-usage), VGPRs + AGPRs (the accumulators) / waves per SIMD, D = 1, 3, 8 (every D:
// DESIGN.md section 10c): NST = 1: 100 + 16 / 4, 122 + 16 / 3, 172 + 16 / 2;  NST = 2: 96 + 32 / 4, 116 + 32 / 3, 166 + 32 / 2;
// NST = 4: 134 + 64 / 2, 160 + 64 / 2, 200 + 64 / 1.  No instantiation uses scratch; the block's LDS is the 32-entry table of
// kuf_exp2_32 (256 bytes).  k_path_gf, k_path_rhs, k_path_fill_v: 14-16 VGPRs, 8 waves per SIMD, no LDS.
// Sample tiles per pass, measured (tools/paths_time.py, profiles/paths_time.log; N = 1e5, M = 512, R = 2048, D = 3, S = 64, kernel and
// table upload): 6.54 / 3.86 / 2.95 ms at one / two / four tiles -- a pass carries four tiles where the call has them.
//
// zigp_sample_paths: per latent  omega = omega0 / ell,  amp = a sqrt(2 var / R);  f_Z = the kernel above on the rows Z with the cosine
// features alone (V = 0: (S, M));  weights from the W = L^-1 of the call's own M x M forward stage (latents_forward), V = W^T t with
//   unwhitened            t = W (u_m + s o eps - f_Z)
//   whitened, diagonal    t = u_m + s o eps - W f_Z
//   whitened, full        t = u_m + tril(L_q) eps - W f_Z
// on the GEMM core (M padded to 128 rows by the identity, S to 128 columns by zeros; the unwhitened V, whose right-hand side holds white
// noise, takes one step of iterative refinement against Kuu: V += W^T W (rhs - Kuu V));  then the kernel on Xnew with the context's mean
// function on f and g_offset on g, and the plane gf = dn_link(g) f (k_path_gf; dn_link of zigp_density.hip as it is).
// Host: path_rows and sample_paths keep their checks, tables and launches; the staging of X, the copy to the host, the call's one
// synchronisation and the refusals' form are stage_inputs, finish_copies and refuse of zigp_rows.h.
#include "zigp_rows.h"
#include <cmath>
#include <cstdlib>

using namespace zigp;

namespace zigp {

constexpr int PT_WAVES = 4, PT_RT = 2;               // waves per block, 16-row tiles per wave
constexpr int PT_ROWS = PT_WAVES * PT_RT * 16;       // rows per block
constexpr int PT_MAXS = 256;
static_assert(PT_MAXS == ZIGP_PATH_MAX_S, "include/zigp.h");

struct PathLat {
  const double* X; int64_t N;           // rows (N, D)
  const double* Zs;                     // (M4, D) inducing inputs scaled by KUF_C / ell_d, zero rows behind M
  const double* omega; const double* phase;   // (R4, D), (R4); zeros behind R
  const double* tab;                    // [sample tile][F][16] weights: kernel features [0, coff), cosines [coff, coff + R4)
  double* out; int64_t ldo;             // out[s * ldo + n]
  int M4, R4, F, coff, kind, S;
  double scale[MAXD], var, lin[MAXD], shift;
};
struct PathArgs { PathLat lat[2]; int ntile; };   // ntile: sample tiles in the table, a multiple of NST

template <int D, int KIND>
__device__ __forceinline__ double path_kval(const double (&zs)[D], const double (&xk)[D], const double* T) {
  double w = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double t = zs[d] - xk[d];
    w = d == 0 ? -t * t : fma(-t, t, w);
  }
  if constexpr (KIND == KERN_RBF) return kuf_exp2_32(w, T);
  else {
    double k, kd = 0.0;
    kuf_matern<KIND, false>(w, T, k, kd);
    return k;
  }
}

template <int D, int NST, int KIND>
__device__ __forceinline__ void path_kernel_groups(const PathLat& a, int t0, const double (&xk)[PT_RT][D], const double* T,
                                                   potrf_d4 (&acc)[PT_RT][NST], int lane) {
  const int g = lane >> 4, i = lane & 15;
  for (int m = g; m < a.M4; m += 4) {      // M4 is a multiple of 4: the trip count is wave-uniform
    double zs[D], wt[NST];
#pragma unroll
    for (int d = 0; d < D; ++d) zs[d] = a.Zs[(int64_t)m * D + d];
#pragma unroll
    for (int j = 0; j < NST; ++j) wt[j] = a.tab[((int64_t)(t0 + j) * a.F + m) * 16 + i];
#pragma unroll
    for (int t = 0; t < PT_RT; ++t) {
      const double v = path_kval<D, KIND>(zs, xk[t], T);
#pragma unroll
      for (int j = 0; j < NST; ++j) acc[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wt[j], v, acc[t][j], 0, 0, 0);
    }
  }
}

template <int D, int NST>
__global__ void __launch_bounds__(64 * PT_WAVES)
k_path_rows(PathArgs pa) {
  const PathLat& a = pa.lat[blockIdx.y];
  __shared__ double T[32];
  if (threadIdx.x < 32) T[threadIdx.x] = a.var * KUF_T[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int64_t row0 = ((int64_t)blockIdx.x * PT_WAVES + wave) * (PT_RT * 16);
  if (row0 >= a.N) return;
  double x[PT_RT][D], xk[PT_RT][D], mp[PT_RT];
  bool valid[PT_RT];
#pragma unroll
  for (int t = 0; t < PT_RT; ++t) {
    const int64_t n = row0 + t * 16 + i;
    valid[t] = n < a.N;
    double m = a.shift;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      x[t][d] = valid[t] ? a.X[n * D + d] : 0.0;
      xk[t][d] = x[t][d] * a.scale[d];
      m = fma(a.lin[d], x[t][d], m);
    }
    mp[t] = m;
  }
  for (int t0 = 0; t0 < pa.ntile; t0 += NST) {
    potrf_d4 acc[PT_RT][NST];
#pragma unroll
    for (int t = 0; t < PT_RT; ++t)
#pragma unroll
      for (int j = 0; j < NST; ++j) acc[t][j] = potrf_d4{0.0, 0.0, 0.0, 0.0};
    if (a.kind == KERN_RBF) path_kernel_groups<D, NST, KERN_RBF>(a, t0, xk, T, acc, lane);
    else if (a.kind == KERN_M32) path_kernel_groups<D, NST, KERN_M32>(a, t0, xk, T, acc, lane);
    else path_kernel_groups<D, NST, KERN_M52>(a, t0, xk, T, acc, lane);
    for (int r = g; r < a.R4; r += 4) {      // R4 is a multiple of 4
      double om[D], wt[NST];
#pragma unroll
      for (int d = 0; d < D; ++d) om[d] = a.omega[(int64_t)r * D + d];
      const double ph = a.phase[r];
#pragma unroll
      for (int j = 0; j < NST; ++j) wt[j] = a.tab[((int64_t)(t0 + j) * a.F + a.coff + r) * 16 + i];
#pragma unroll
      for (int t = 0; t < PT_RT; ++t) {
        double arg = om[0] * x[t][0];
#pragma unroll
        for (int d = 1; d < D; ++d) arg = fma(om[d], x[t][d], arg);
        const double v = cos(arg + ph);
#pragma unroll
        for (int j = 0; j < NST; ++j) acc[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wt[j], v, acc[t][j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < PT_RT; ++t) {
      if (!valid[t]) continue;
      const int64_t n = row0 + t * 16 + i;
#pragma unroll
      for (int j = 0; j < NST; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int s = (t0 + j) * 16 + 4 * q + g;
          if (s < a.S) a.out[(int64_t)s * a.ldo + n] = acc[t][j][q] + mp[t];
        }
    }
  }
}

// gf = dn_link(g) f, element by element over the (S, N) planes
__global__ void __launch_bounds__(256)
k_path_gf(const double* __restrict__ f, const double* __restrict__ gl, double* __restrict__ gf, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < n) gf[idx] = __dmul_rn(dn_link(gl[idx]), f[idx]);
}

// The right-hand side of the weights, (Mp, Sp) row-major, zero outside (M, S).  mode = Param:
//   Diag       u_m + s_m E[m][s] - FT[s][m]        (FT: f_Z as the path kernel wrote it, (Sp, Mp))
//   White      u_m + s_m E[m][s] - G[m][s]         (G = W f_Z)
//   WhiteFull  u_m + H[m][s] - G[m][s]             (H = tril(L_q) E)
__global__ void __launch_bounds__(256)
k_path_rhs(int mode, const double* __restrict__ u, const double* __restrict__ sd, const double* __restrict__ E, const double* __restrict__ FT,
           const double* __restrict__ G, const double* __restrict__ H, int M, int S, int64_t Mp, int64_t Sp, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Mp * Sp) return;
  const int64_t m = idx / Sp, s = idx - m * Sp;
  double v = 0.0;
  if (m < M && s < S) {
    const double head = mode == 2 ? u[m] + H[idx] : fma(sd[m], E[idx], u[m]);
    v = head - (mode == 0 ? FT[s * Mp + m] : G[idx]);
  }
  out[idx] = v;
}

// out = a + alpha b, element by element (out may be a)
__global__ void __launch_bounds__(256)
k_path_axpy(const double* a, double alpha, const double* __restrict__ b, int64_t n, double* out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < n) out[idx] = fma(alpha, b[idx], a[idx]);
}

// The kernel features' part of a weight table from V (Mp, Sp) row-major: tab[tile][m][i] = V[m][16 tile + i] for m < M and 16 tile + i < S, else 0
__global__ void __launch_bounds__(256)
k_path_fill_v(const double* __restrict__ V, int M, int S, int M4, int F, int ntile, int64_t Sp, double* __restrict__ tab) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)ntile * M4 * 16) return;
  const int i = (int)(idx & 15);
  const int64_t q = idx >> 4;
  const int m = (int)(q % M4), tile = (int)(q / M4), s = tile * 16 + i;
  tab[((int64_t)tile * F + m) * 16 + i] = (m < M && s < S) ? V[(int64_t)m * Sp + s] : 0.0;
}

}  // namespace zigp

namespace {

// Sample tiles per pass: 4 where the call has that many, else 2 or 1 (tools/paths_time.py is the measurement; env ZIGP_PATH_TILES = 1, 2
// or 4 caps it for that tool).  The choice moves no bit of the result.
int path_tiles_per_pass(int S) {
  const int ntile = (S + 15) / 16;
  int cap = 4;
  if (const char* e = getenv("ZIGP_PATH_TILES")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) cap = v; }
  int nst = ntile >= 4 ? 4 : ntile >= 2 ? 2 : 1;
  return std::min(nst, cap);
}

template <int D>
int path_launch_d(zigp_ctx* c, const PathArgs& pa, int nlat, int nst, int64_t maxN) {
  const dim3 grid((unsigned)ceil_div(maxN, PT_ROWS), (unsigned)nlat), block(64 * PT_WAVES);
  if (nst == 4) hipLaunchKernelGGL((k_path_rows<D, 4>), grid, block, 0, c->stream, pa);
  else if (nst == 2) hipLaunchKernelGGL((k_path_rows<D, 2>), grid, block, 0, c->stream, pa);
  else hipLaunchKernelGGL((k_path_rows<D, 1>), grid, block, 0, c->stream, pa);
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
int path_launch(zigp_ctx* c, int D, const PathArgs& pa, int nlat, int nst) {
  int64_t maxN = 0;
  for (int h = 0; h < nlat; ++h) maxN = std::max(maxN, pa.lat[h].N);
  if (maxN <= 0) return 0;
  switch (D) {
    case 1: return path_launch_d<1>(c, pa, nlat, nst, maxN);
    case 2: return path_launch_d<2>(c, pa, nlat, nst, maxN);
    case 3: return path_launch_d<3>(c, pa, nlat, nst, maxN);
    case 4: return path_launch_d<4>(c, pa, nlat, nst, maxN);
    case 5: return path_launch_d<5>(c, pa, nlat, nst, maxN);
    case 6: return path_launch_d<6>(c, pa, nlat, nst, maxN);
    case 7: return path_launch_d<7>(c, pa, nlat, nst, maxN);
    case 8: return path_launch_d<8>(c, pa, nlat, nst, maxN);
    default: return fail_arg(c, "the path kernel covers D in [1, 8]");
  }
}

bool path_all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}
int path_check_dims(zigp_ctx* c, const std::string& w, int D, int S, int64_t N) {
  if (D < 1) return refuse(c, w, "D must be positive");
  if (D > MAXD) return refuse(c, w, "D = " + std::to_string(D) + ": the path kernel covers D in [1, 8] (the wide path is not built)");
  if (S < 1 || S > PT_MAXS) return refuse(c, w, "S = " + std::to_string(S) + " must be in [1, 256] (ZIGP_PATH_MAX_S)");
  if (N < 0) return refuse(c, w, "N is negative");
  return 0;
}
// a table: NULL or a non-finite entry is refused by the table's name
int path_check_table(zigp_ctx* c, const std::string& w, const char* name, const double* p, size_t n) {
  if (n == 0) return 0;
  if (!p) return refuse(c, w, std::string(name) + " is NULL");
  if (!path_all_finite(p, n)) return refuse(c, w, std::string(name) + " has a non-finite entry");
  return 0;
}

// The sizes of one latent's device tables, in doubles
struct PathDims { int M4, R4, F; };
PathDims path_dims(int M, int R) { PathDims d; d.M4 = (int)round_up(M, 4); d.R4 = (int)round_up(std::max(R, 0), 4); d.F = d.M4 + d.R4; return d; }

// zigp_path_rows and zigp_path_rows_device
int path_rows(zigp_ctx* c, const char* who, const zigp_path_latent* lat, int nlat, int D, int S, const double* X, int64_t N, double* out, bool on_device) {
  if (!c) return ZIGP_EARG;
  const std::string w(who);
  if (!lat) return refuse(c, w, "lat is NULL");
  if (nlat != 1 && nlat != 2) return refuse(c, w, "nlat must be 1 or 2");
  ZIGP_TRY(path_check_dims(c, w, D, S, N));
  for (int h = 0; h < nlat; ++h) {
    const zigp_path_latent& q = lat[h];
    if (q.kind != ZIGP_KERN_RBF && q.kind != ZIGP_KERN_MATERN32 && q.kind != ZIGP_KERN_MATERN52)
      return refuse(c, w, "kind is not a ZIGP_KERN_* value");
    if (q.M < 1) return refuse(c, w, "M must be positive");
    if (q.R < 0) return refuse(c, w, "R is negative");
    ZIGP_TRY(path_check_table(c, w, "Z", q.Z, (size_t)q.M * D));
    ZIGP_TRY(path_check_table(c, w, "ell", q.ell, D));
    ZIGP_TRY(path_check_table(c, w, "V", q.V, (size_t)q.M * S));
    ZIGP_TRY(path_check_table(c, w, "omega", q.omega, (size_t)q.R * D));
    ZIGP_TRY(path_check_table(c, w, "phase", q.phase, q.R));
    ZIGP_TRY(path_check_table(c, w, "amp", q.amp, (size_t)q.R * S));
    if (q.lin && !path_all_finite(q.lin, D)) return refuse(c, w, "lin has a non-finite entry");
    if (!std::isfinite(q.shift)) return refuse(c, w, "shift is not finite");
    if (!(q.var > 0 && std::isfinite(q.var))) return refuse(c, w, "var must be positive and finite");
    for (int d = 0; d < D; ++d)
      if (!(q.ell[d] > 0)) return refuse(c, w, "ell must be positive");
  }
  if (N > 0 && (!X || !out)) return refuse(c, w, "X or out is NULL");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device) ZIGP_TRY(require_device_ptrs(c, {X, out}, (w + ": X and out must be device memory of the context's GPU").c_str()));
  ZIGP_TRY(begin_staged_call(c));
  const int nst = path_tiles_per_pass(S), ntile = (int)round_up((S + 15) / 16, nst);
  // one staged image: per latent [Zs | omega | phase | table]
  size_t off[2][4], total = 0;
  PathDims dm[2];
  for (int h = 0; h < nlat; ++h) {
    dm[h] = path_dims(lat[h].M, lat[h].R);
    off[h][0] = total; total += (size_t)dm[h].M4 * D;
    off[h][1] = total; total += (size_t)dm[h].R4 * D;
    off[h][2] = total; total += (size_t)dm[h].R4;
    off[h][3] = total; total += (size_t)ntile * dm[h].F * 16;
  }
  ZIGP_ENSURE(c, c->path_tab, total);
  ZIGP_PINNED(c, img, total);
  memset(img, 0, sizeof(double) * total);
  PathArgs pa{};
  pa.ntile = ntile;
  for (int h = 0; h < nlat; ++h) {
    const zigp_path_latent& q = lat[h];
    const KufHyp kh = make_kuf_hyp(q.ell, q.var, D);
    for (int m = 0; m < q.M; ++m)
      for (int d = 0; d < D; ++d) img[off[h][0] + (size_t)m * D + d] = q.Z[(size_t)m * D + d] * kh.scale[d];
    if (q.R > 0) {
      memcpy(img + off[h][1], q.omega, sizeof(double) * q.R * D);
      memcpy(img + off[h][2], q.phase, sizeof(double) * q.R);
    }
    double* tab = img + off[h][3];
    for (int s = 0; s < S; ++s) {
      double* tt = tab + (size_t)(s >> 4) * dm[h].F * 16 + (s & 15);
      for (int m = 0; m < q.M; ++m) tt[(size_t)m * 16] = q.V[(size_t)m * S + s];
      for (int r = 0; r < q.R; ++r) tt[(size_t)(dm[h].M4 + r) * 16] = q.amp[(size_t)r * S + s];
    }
    PathLat& a = pa.lat[h];
    a.N = N; a.Zs = c->path_tab.p + off[h][0]; a.omega = c->path_tab.p + off[h][1]; a.phase = c->path_tab.p + off[h][2];
    a.tab = c->path_tab.p + off[h][3];
    a.ldo = N; a.M4 = dm[h].M4; a.R4 = dm[h].R4; a.F = dm[h].F; a.coff = dm[h].M4; a.kind = q.kind; a.S = S;
    for (int d = 0; d < MAXD; ++d) { a.scale[d] = kh.scale[d]; a.lin[d] = (q.lin && d < D) ? q.lin[d] : 0.0; }
    a.var = q.var; a.shift = q.shift;
  }
  ZIGP_HIP(c, hipMemcpyAsync(c->path_tab.p, img, sizeof(double) * total, hipMemcpyHostToDevice, c->stream));
  const double* dX = nullptr;
  ZIGP_TRY(stage_inputs(c, X, N, D, on_device, &dX));
  if (!on_device) ZIGP_ENSURE(c, c->path_out, (size_t)nlat * S * N);
  double* dout = on_device ? out : c->path_out.p;
  for (int h = 0; h < nlat; ++h) { pa.lat[h].X = dX; pa.lat[h].out = dout + (size_t)h * S * N; }
  ZIGP_TRY(path_launch(c, D, pa, nlat, nst));
  return finish_copies(c, {{on_device ? nullptr : out, dout, (size_t)nlat * S * N}});
}

int path_check_draw(zigp_ctx* c, const std::string& w, const char* tag, const zigp_path_draw* dr, int M, int D, int S) {
  const std::string t(tag);
  if (!dr) return refuse(c, w, "draw_" + t + " is NULL");
  if (dr->R < 0) return refuse(c, w, "draw_" + t + ": R is negative");
  ZIGP_TRY(path_check_table(c, w, ("draw_" + t + ".omega0").c_str(), dr->omega0, (size_t)dr->R * D));
  ZIGP_TRY(path_check_table(c, w, ("draw_" + t + ".phase").c_str(), dr->phase, dr->R));
  ZIGP_TRY(path_check_table(c, w, ("draw_" + t + ".a").c_str(), dr->a, (size_t)dr->R * S));
  ZIGP_TRY(path_check_table(c, w, ("draw_" + t + ".eps").c_str(), dr->eps, (size_t)M * S));
  return 0;
}

// C (Mp, Sp) = op(A) B over the full tile list: A = W or L_q ((Mp, Mp) row-major; transposed: W^T), B (Mp, Sp) row-major or -- bt -- (Sp, Mp)
int path_gemm(zigp_ctx* c, bool at, bool bt, const double* A, const double* B, double* C, int Mp, int Sp) {
  TileList tl;
  ZIGP_TRY(tiles_full(c, Mp / BM, Sp / BN, Mp / BK, tl));
  GemmArgs g = mk_args(A, Mp, B, bt ? Mp : Sp, C, Sp);
  if (!at && !bt) return run_gemm<LAY_KCONTIG, LAY_MNCONTIG, false>(c, tl, g, EpiStore());
  if (at && !bt) return run_gemm<LAY_MNCONTIG, LAY_MNCONTIG, false>(c, tl, g, EpiStore());
  if (!at && bt) return run_gemm<LAY_KCONTIG, LAY_KCONTIG, false>(c, tl, g, EpiStore());
  return run_gemm<LAY_MNCONTIG, LAY_KCONTIG, false>(c, tl, g, EpiStore());
}

// The tap sink of the weight-stage hooks (zigp_test_path_weights, zigp_test_kron_path_weights; include/zigp_diag.h).  A tap is a
// device-to-device copy enqueued on the call's stream right behind the launch that produces the value, into a buffer of its own; flush()
// downloads them once the stream is idle.  Host code only: a product call passes no sink and enqueues exactly what it did before.
struct PathTap {
  struct Snap { double* host; DevBuf dev; size_t n; };
  std::vector<Snap> snaps;
  int snap(zigp_ctx* c, double* host, const double* dev, size_t n) {
    if (!host || n == 0) return 0;
    snaps.emplace_back();
    Snap& q = snaps.back();
    q.host = host; q.n = n;
    ZIGP_ENSURE(c, q.dev, n);
    ZIGP_HIP(c, hipMemcpyAsync(q.dev.p, dev, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  int sentinel(zigp_ctx* c, double* dev, size_t n) {
    ZIGP_HIP(c, hipMemsetAsync(dev, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * n, c->stream));
    return 0;
  }
  int flush(zigp_ctx* c) {      // the stream is idle
    for (Snap& q : snaps) ZIGP_HIP(c, hipMemcpy(q.host, q.dev.p, sizeof(double) * q.n, hipMemcpyDeviceToHost));
    return 0;
  }
};
struct DensePathTap : PathTap { const zigp_stage_path_weights* s; int64_t facts[ZIGP_PWF_COUNT]; };
// PW_SNAP(field, device pointer, count): latent h's tap of that name; a no-op without a sink
#define PW_SNAP(field, dev, n) do { if (tap) ZIGP_TRY(tap->snap(c, tap->s->lat[h].field, (dev), (n))); } while (0)

// The weight stage of zigp_sample_paths behind the call's own M x M forward stage: the device tables of both latents, f_Z by the path
// kernel on the rows Z, V = W^T t on the GEMM core and the kernel features' part of the weight table.  pa comes back as the argument record
// of the path launch at Xnew (X, N, out, ldo, the mean part are the caller's to set).
int path_weight_stage(zigp_ctx* c, Param par, const HostLatent (&hl)[2], const zigp_path_draw* const (&dr)[2], int D, int S, int nst, PathArgs& pa,
                      DensePathTap* tap) {
  const int ntile = (int)round_up((S + 15) / 16, nst);
  const int64_t Sp = round_up(S, BN);
  // device tables per latent: [omega | phase | table] staged from the host, then [E | FT | A | B | V] work matrices
  size_t off[2][8], total = 0, staged = 0;
  PathDims dm[2];
  for (int h = 0; h < 2; ++h) {
    dm[h] = path_dims(hl[h].M, dr[h]->R);
    const size_t Mp = c->lat[h].Mp;
    off[h][0] = total; total += (size_t)dm[h].R4 * D;
    off[h][1] = total; total += (size_t)dm[h].R4;
    off[h][2] = total; total += (size_t)ntile * dm[h].F * 16;
    off[h][3] = total; total += Mp * Sp;      // E (Mp, Sp)
  }
  staged = total;
  for (int h = 0; h < 2; ++h) {
    const size_t Mp = c->lat[h].Mp;
    off[h][4] = total; total += Mp * Sp;      // FT (Sp, Mp)
    off[h][5] = total; total += Mp * Sp;      // A
    off[h][6] = total; total += Mp * Sp;      // B
    off[h][7] = total; total += Mp * Sp;      // V
  }
  ZIGP_ENSURE(c, c->path_tab, total);
  double* base = c->path_tab.p;
  ZIGP_PINNED(c, img, staged);
  memset(img, 0, sizeof(double) * staged);
  pa = PathArgs{};
  pa.ntile = ntile;
  for (int h = 0; h < 2; ++h) {
    const int R = dr[h]->R, M = hl[h].M;
    const KufHyp kh = make_kuf_hyp(hl[h].ell, hl[h].var, D);
    for (int r = 0; r < R; ++r) {
      for (int d = 0; d < D; ++d) img[off[h][0] + (size_t)r * D + d] = dr[h]->omega0[(size_t)r * D + d] / hl[h].ell[d];
      img[off[h][1] + r] = dr[h]->phase[r];
    }
    const double ampl = R > 0 ? sqrt(2.0 * hl[h].var / R) : 0.0;
    double* tab = img + off[h][2];
    for (int s = 0; s < S; ++s) {
      double* tt = tab + (size_t)(s >> 4) * dm[h].F * 16 + (s & 15);
      for (int r = 0; r < R; ++r) tt[(size_t)(dm[h].M4 + r) * 16] = dr[h]->a[(size_t)r * S + s] * ampl;
    }
    double* E = img + off[h][3];
    for (int m = 0; m < M; ++m) memcpy(E + (size_t)m * Sp, dr[h]->eps + (size_t)m * S, sizeof(double) * S);
    PathLat& a = pa.lat[h];
    a.Zs = c->lat[h].Zs.p; a.omega = base + off[h][0]; a.phase = base + off[h][1]; a.tab = base + off[h][2];
    a.M4 = dm[h].M4; a.R4 = dm[h].R4; a.F = dm[h].F; a.coff = dm[h].M4; a.kind = hl[h].kind; a.S = S;
    for (int d = 0; d < MAXD; ++d) { a.scale[d] = kh.scale[d]; a.lin[d] = 0.0; }
    a.var = hl[h].var; a.shift = 0.0;
  }
  ZIGP_HIP(c, hipMemcpyAsync(base, img, sizeof(double) * staged, hipMemcpyHostToDevice, c->stream));
  ZIGP_HIP(c, hipMemsetAsync(base + staged, 0, sizeof(double) * (total - staged), c->stream));
  if (tap) {      // the hook: A, B and V are written completely by their launches (FT is not: the path kernel writes (S, M) of it)
    tap->facts[ZIGP_PWF_MODE] = par == Param::Diag ? 0 : is_full(par) ? 2 : 1;
    tap->facts[ZIGP_PWF_SP] = Sp; tap->facts[ZIGP_PWF_NST] = nst; tap->facts[ZIGP_PWF_NTILE] = ntile;
    for (int h = 0; h < 2; ++h) {
      const size_t Mp = c->lat[h].Mp;
      tap->facts[ZIGP_PWF_MP + h] = (int64_t)Mp; tap->facts[ZIGP_PWF_M4 + h] = dm[h].M4; tap->facts[ZIGP_PWF_R4 + h] = dm[h].R4;
      tap->facts[ZIGP_PWF_F + h] = dm[h].F;
      ZIGP_TRY(tap->sentinel(c, base + off[h][5], 3 * Mp * Sp));
      PW_SNAP(Kuu, c->lat[h].Kuu.p, Mp * Mp); PW_SNAP(W, c->lat[h].W.p, Mp * Mp);
      if (is_full(par)) PW_SNAP(Lq, c->lat[h].Lq.p, Mp * Mp);
      PW_SNAP(u, c->lat[h].u.p, Mp); PW_SNAP(s, c->lat[h].s.p, Mp);
      PW_SNAP(E, base + off[h][3], Mp * Sp);
    }
  }

  // f_Z: the cosine features alone on the rows Z (V = 0: no kernel group runs), written as (S, M) with row stride Mp
  PathArgs pz = pa;
  for (int h = 0; h < 2; ++h) {
    PathLat& a = pz.lat[h];
    a.X = c->lat[h].Z.p; a.N = hl[h].M; a.M4 = 0; a.out = base + off[h][4]; a.ldo = c->lat[h].Mp;
  }
  ZIGP_TRY(path_launch(c, D, pz, 2, nst));

  // V = W^T t on the GEMM core
  for (int h = 0; h < 2; ++h) {
    Latent& lt = c->lat[h];
    const int Mp = lt.Mp, M = hl[h].M;
    const size_t ms = (size_t)Mp * Sp;
    double *E = base + off[h][3], *FT = base + off[h][4], *A = base + off[h][5], *B = base + off[h][6], *V = base + off[h][7];
    const dim3 grid((unsigned)ceil_div((int64_t)Mp * Sp, 256));
    PW_SNAP(FT, FT, ms);
    if (par == Param::Diag) {
      hipLaunchKernelGGL(k_path_rhs, grid, dim3(256), 0, c->stream, 0, lt.u.p, lt.s.p, E, FT, nullptr, nullptr, M, S, (int64_t)Mp, Sp, A);
      ZIGP_HIP(c, hipGetLastError());
      PW_SNAP(rhs, A, ms);
      ZIGP_TRY(path_gemm(c, false, false, lt.W.p, A, B, Mp, (int)Sp));      // t = W (u + s o eps - f_Z)
      PW_SNAP(t, B, ms);
      ZIGP_TRY(path_gemm(c, true, false, lt.W.p, B, V, Mp, (int)Sp));       // V = W^T t
      PW_SNAP(V0, V, ms);
      // One step of iterative refinement against Kuu itself.  The right-hand side holds the white noise s o eps, so V is of the size of
      // 1 / jitter, and a path is k(x, Z) V = (k(x, Z) Kuu^-1)(rhs - residual): what reaches the path is the RESIDUAL of V.  Through the
      // explicit W it is ~cond(L) eps |Kuu| |V| (measured 9.6e-7 of a path at cond(Kuu) 4e8, where the restatement's triangular solves
      // are at 1.4e-8); after V += W^T W (rhs - Kuu V) it is that of a backward-stable solve.  The step is held by the solve tier of
      // tests/test_gpu_path_weight_stages.py: max |rhs - Kuu V| <= 8 x SciPy's Cholesky solve (65 x before the step, 0.98 x after it there).
      ZIGP_TRY(path_gemm(c, false, false, lt.Kuu.p, V, FT, Mp, (int)Sp));   // Kuu V  (f_Z has no reader left: its buffer as (Mp, Sp))
      PW_SNAP(KV, FT, ms);
      hipLaunchKernelGGL(k_path_axpy, grid, dim3(256), 0, c->stream, A, -1.0, FT, (int64_t)Mp * Sp, A);       // residual
      ZIGP_HIP(c, hipGetLastError());
      PW_SNAP(res, A, ms);
      ZIGP_TRY(path_gemm(c, false, false, lt.W.p, A, B, Mp, (int)Sp));
      PW_SNAP(t2, B, ms);
      ZIGP_TRY(path_gemm(c, true, false, lt.W.p, B, FT, Mp, (int)Sp));      // the correction
      PW_SNAP(cor, FT, ms);
      hipLaunchKernelGGL(k_path_axpy, grid, dim3(256), 0, c->stream, V, 1.0, FT, (int64_t)Mp * Sp, V);
      ZIGP_HIP(c, hipGetLastError());
    } else {
      ZIGP_TRY(path_gemm(c, false, true, lt.W.p, FT, A, Mp, (int)Sp));      // G = W f_Z
      PW_SNAP(G, A, ms);
      if (is_full(par)) {
        ZIGP_TRY(path_gemm(c, false, false, lt.Lq.p, E, B, Mp, (int)Sp));   // H = tril(L_q) eps
        PW_SNAP(H, B, ms);
      }
      hipLaunchKernelGGL(k_path_rhs, grid, dim3(256), 0, c->stream, is_full(par) ? 2 : 1, lt.u.p, lt.s.p, E, nullptr, A, B, M, S, (int64_t)Mp, Sp, FT);
      ZIGP_HIP(c, hipGetLastError());
      PW_SNAP(rhs, FT, ms);
      ZIGP_TRY(path_gemm(c, true, false, lt.W.p, FT, V, Mp, (int)Sp));      // V = W^T t  (t overwrote f_Z, which has no reader left)
    }
    PW_SNAP(V, V, ms);
    if (tap)      // k_path_fill_v writes every kernel row of the table
      for (int tile = 0; tile < ntile; ++tile) ZIGP_TRY(tap->sentinel(c, base + off[h][2] + (size_t)tile * dm[h].F * 16, (size_t)dm[h].M4 * 16));
    const int64_t nfill = (int64_t)ntile * dm[h].M4 * 16;
    hipLaunchKernelGGL(k_path_fill_v, dim3((unsigned)ceil_div(nfill, 256)), dim3(256), 0, c->stream, V, M, S, dm[h].M4, dm[h].F, ntile, Sp,
                       base + off[h][2]);
    ZIGP_HIP(c, hipGetLastError());
    PW_SNAP(tab, base + off[h][2], (size_t)ntile * dm[h].F * 16);
  }
  return 0;
}

// The call's own M x M forward stage: Kuu, L, W = L^-1 (and the masked L_q of a full-covariance call); *hinfo holds the factorisation's
// status after the call's synchronisation
int paths_forward(zigp_ctx* c, const HostLatent (&hl)[2], int D, double jitter, Param par, int** hinfo) {
  ZIGP_TRY(begin_staged_call(c));
  ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  ZIGP_TRY(latents_upload(c, hl, D, par));
  ZIGP_TRY(fork_side(c, c->ev_fork, c->stream2));
  ZIGP_TRY(latents_forward(c, hl, D, jitter, par, false, false, nullptr, nullptr));
  ZIGP_TRY(join_side(c, c->ev_join, c->stream2));
  return request_info(c, hinfo);
}

// zigp_sample_paths and zigp_sample_paths_device
int sample_paths(zigp_ctx* c, const char* who, const zigp_params* p, const double* X, int64_t N, double jitter, double g_offset,
                 const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int S, double* out3, bool on_device) {
  if (!c) return ZIGP_EARG;
  const std::string w(who);
  if (p && p->D > MAXD && p->D <= ZIGP_MAX_D) ZIGP_TRY(path_check_dims(c, w, p->D, 1, 0));     // names D before validate_params speaks of the wide kernels
  ZIGP_TRY(validate_params(c, p));
  const int D = p->D;
  ZIGP_TRY(path_check_dims(c, w, D, S, N));
  ZIGP_TRY(path_check_draw(c, w, "f", draw_f, p->Mf, D, S));
  ZIGP_TRY(path_check_draw(c, w, "g", draw_g, p->Mg, D, S));
  if (!std::isfinite(g_offset)) return refuse(c, w, "g_offset is not finite");
  if (N > 0 && (!X || !out3)) return refuse(c, w, "Xnew or out3 is NULL");
  if (N == 0) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device) ZIGP_TRY(require_device_ptrs(c, {X, out3}, (w + ": Xnew and out3 must be device memory of the context's GPU").c_str()));

  // the call's own M x M forward stage: Kuu, L, W = L^-1 (and the masked L_q of a full-covariance call)
  const Param par = param_of(c);
  HostLatent hl[2] = {{p->Mf, p->Zf, p->u_fm, p->u_fs_sqrt, p->ell_f, p->var_f, c->kern[0]},
                      {p->Mg, p->Zg, p->u_gm, p->u_gs_sqrt, p->ell_g, p->var_g, c->kern[1]}};
  const zigp_path_draw* dr[2] = {draw_f, draw_g};
  int* hinfo = nullptr;
  ZIGP_TRY(paths_forward(c, hl, D, jitter, par, &hinfo));

  const int nst = path_tiles_per_pass(S);
  PathArgs pa{};
  ZIGP_TRY(path_weight_stage(c, par, hl, dr, D, S, nst, pa, nullptr));

  // the paths at Xnew: the context's mean function on f, g_offset on g
  const double* dX = nullptr;
  ZIGP_TRY(stage_inputs(c, X, N, D, on_device, &dX));
  if (!on_device) ZIGP_ENSURE(c, c->path_out, (size_t)3 * S * N);
  double* dout = on_device ? out3 : c->path_out.p;
  for (int h = 0; h < 2; ++h) {
    PathLat& a = pa.lat[h];
    a.X = dX; a.N = N; a.out = dout + (size_t)h * S * N; a.ldo = N;
  }
  if (c->mean_on) {
    pa.lat[0].shift = c->mean_b;
    for (int d = 0; d < D; ++d) pa.lat[0].lin[d] = c->mean_a[d];
  }
  pa.lat[1].shift = g_offset;
  ZIGP_TRY(path_launch(c, D, pa, 2, nst));
  const int64_t SN = (int64_t)S * N;
  hipLaunchKernelGGL(k_path_gf, dim3((unsigned)ceil_div(SN, 256)), dim3(256), 0, c->stream, dout, dout + SN, dout + 2 * SN, SN);
  ZIGP_HIP(c, hipGetLastError());
  ZIGP_TRY(finish_copies(c, {{on_device ? nullptr : out3, dout, (size_t)3 * SN}}));
  prof_collect(c);
  return info_result(c, hinfo, "Kuu");
}

}  // namespace

extern "C" {

int zigp_path_rows(zigp_ctx* c, const zigp_path_latent* lat, int32_t nlat, int32_t D, int32_t S, const double* X, int64_t N, double* out) {
  return path_rows(c, "zigp_path_rows", lat, nlat, D, S, X, N, out, false);
}

int zigp_path_rows_device(zigp_ctx* c, const zigp_path_latent* lat, int32_t nlat, int32_t D, int32_t S, const double* dX, int64_t N, double* d_out) {
  return path_rows(c, "zigp_path_rows_device", lat, nlat, D, S, dX, N, d_out, true);
}

int zigp_sample_paths(zigp_ctx* c, const zigp_params* p, const double* Xnew, int64_t N, double jitter, double g_offset,
                      const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* out3) {
  return sample_paths(c, "zigp_sample_paths", p, Xnew, N, jitter, g_offset, draw_f, draw_g, S, out3, false);
}

int zigp_sample_paths_device(zigp_ctx* c, const zigp_params* p, const double* dXnew, int64_t N, double jitter, double g_offset,
                             const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* d_out3) {
  return sample_paths(c, "zigp_sample_paths_device", p, dXnew, N, jitter, g_offset, draw_f, draw_g, S, d_out3, true);
}

// The weight stage of zigp_sample_paths through path_weight_stage itself, behind the call's own forward stage, with its device buffers
// snapshot (DensePathTap); the paths at Xnew are not run.  The checks are those of sample_paths that do not concern rows.
int zigp_test_path_weights(zigp_ctx* c, const zigp_stage_path_weights* s) {
  if (!c) return ZIGP_EARG;
  const std::string w("zigp_test_path_weights");
  if (!s) return refuse(c, w, "the record is NULL");
  const zigp_params* p = s->p;
  if (p && p->D > MAXD && p->D <= ZIGP_MAX_D) ZIGP_TRY(path_check_dims(c, w, p->D, 1, 0));
  ZIGP_TRY(validate_params(c, p));
  const int D = p->D, S = s->S;
  ZIGP_TRY(path_check_dims(c, w, D, S, 0));
  ZIGP_TRY(path_check_draw(c, w, "f", s->draw_f, p->Mf, D, S));
  ZIGP_TRY(path_check_draw(c, w, "g", s->draw_g, p->Mg, D, S));
  if (!(s->jitter >= 0)) return refuse(c, w, "jitter must be >= 0");
  ZIGP_HIP(c, hipSetDevice(c->device));
  const Param par = param_of(c);
  HostLatent hl[2] = {{p->Mf, p->Zf, p->u_fm, p->u_fs_sqrt, p->ell_f, p->var_f, c->kern[0]},
                      {p->Mg, p->Zg, p->u_gm, p->u_gs_sqrt, p->ell_g, p->var_g, c->kern[1]}};
  const zigp_path_draw* dr[2] = {s->draw_f, s->draw_g};
  int* hinfo = nullptr;
  ZIGP_TRY(paths_forward(c, hl, D, s->jitter, par, &hinfo));
  DensePathTap tap;
  tap.s = s;
  memset(tap.facts, 0, sizeof(tap.facts));
  PathArgs pa{};
  ZIGP_TRY(path_weight_stage(c, par, hl, dr, D, S, path_tiles_per_pass(S), pa, &tap));
  ZIGP_TRY(finish_copies(c, {}));
  ZIGP_TRY(tap.flush(c));
  if (s->facts) memcpy(s->facts, tap.facts, sizeof(tap.facts));
  return info_result(c, hinfo, "Kuu");
}

}  // extern "C"
