// Fused Kronecker (space x time) path for small inducing grids (every factor <= 16 * KF_NBMAX points): scripts/onoff.py:143-319,
// onofftf/main.py:350-387, onofftf/onoffpred.py:127-200.  Same factored algebra as zigp_kron.hip (see its header), but nothing
// of size O(M N) ever reaches HBM: a WAVE owns a tile of 16 points and keeps every per-point vector in registers in the
// operand layout of v_mfma_f64_16x16x4 (round 4; rounds 2-3: four v_mfma_f64_4x4x4 per product), whose B operand and D result share one lane layout
//     V[q] of lane l  =  V(row 4 q + l / 16, point l % 16)
// so the result of one product feeds the next one with no shuffle or LDS round trip.  The M_p x M_p / M_0 x M_1 matrices
// (P_p = K_p^-1, Alpha, S2 and the transposes) are read from global memory (L1 / L2 resident: 8 KB each at 32 x 32) in
// A-FRAGMENT ORDER, one coalesced 32-byte load per lane and 16 x 16 x 4 product.  Launches per step:
//   k_kf_factor   one workgroup per factor: K_p + jitter, Cholesky + triangular inverse in LDS, P_p = W^T W, logdet, diag(P_p)
//   k_kf_latent   one workgroup per latent: Alpha = P0 U P1, T0 = U P1, T1 = P0 U, KL scalars, fragment images
//   k_kf_forward  q0, q1, mean, S-term per point (part[4][N])                      (kron_inf value, scripts/onoff.py:186-213)
//   k_kron_pointwise / k_kron_head_pointwise (zigp_kron.hip)                       (probit moments, likelihood, reverse pass)
//   k_kf_backward recomputes the forward tile, hand-derived reverse pass; the sums over points (dAlpha, dS2, dP_p and the
//                 kernel-cotangent moments) accumulate in MFMA accumulators across the wave's tiles -> one partial per wave
//   k_kf_reduce   fixed-order sum of the per-wave partials (+ one workgroup for the sums of the point-wise block partials;
//                 value-only steps launch k_kron_pw_reduce for those instead)
//   k_kf_finish   one workgroup per latent: the M x M reverse pass (dU, dP_p -> dK_p -> dZ, dell, dvar; KL gradient)
// plus ONE staged host->device copy (parameters + minibatch) and ONE device->host copy (results).
#include "zigp_host.h"

namespace zigp {

constexpr int KF_NBMAX = 2;       // 16-row blocks per factor handled by the register-resident kernels (M_p <= 32)
constexpr int KF_LD = 18;         // LDS row stride (doubles) of a [rows][16 points] tile: A- and B-fragment reads are conflict free
constexpr int KF_WAVES = 4;       // waves per workgroup (each wave works alone on its own tiles)

struct KfFac {
  int M, nb, D, col0;
  const double* hyp;        // this factor's record of the device hyperparameter block (KH_INV, KH_ZC, KH_VAR; zigp_kernels.h): 1 / ell, the centre
                            // zc of the moment sums (mid-range of Z_p: sum t (x - z)^k is rebuilt from sum t (x - zc)^k), the variance
  const double* Zs;         // [16 nb][D] inducing inputs divided by the lengthscales, zero rows beyond M (written by k_kf_factor)
  const double* PF;         // P_p in A-fragment order [nb][4 nb][16][4]
};
struct KfLat {
  KfFac f[2];
  const double *AlF, *S2F;      // [nb0][4 nb1][16][4]   rows = factor-0 index, k = factor-1 index
  const double *AlTF, *S2TF;    // [nb1][4 nb0][16][4]   the transposes
  double* part;                 // [4][Npad]: q0, q1, mean, S-term
  const double *gm, *gv, *dq0, *dq1;   // [Npad] cotangents from the point-wise kernel
  double* acc;                  // [waves][KF_ACC_BLOCKS][4][64] per-wave partial sums
  double* spill;                // larger grids: per-tile operand records of the sums over points (zigp_kronl.h)
};
struct KfArgs {
  KfLat lat[2];
  const double* X; int64_t N, Npad; int ldx;
  int tpw;        // tiles per wave
  int lat0;       // first latent of this launch (latents with different block counts are launched separately)
  int ntiles;     // Npad / 16
  int tile0, tile1;   // k_kfl_backward: the tile range of this launch (its spill records are numbered from tile0)
};

// accumulator blocks of the backward kernel (16 x 16 each), compile-time layout for KF_NBMAX
constexpr int KF_B_AL = 0;
constexpr int KF_B_S2 = KF_B_AL + KF_NBMAX * KF_NBMAX;
constexpr int KF_B_P0 = KF_B_S2 + KF_NBMAX * KF_NBMAX;
constexpr int KF_B_P1 = KF_B_P0 + KF_NBMAX * KF_NBMAX;
constexpr int KF_B_K0 = KF_B_P1 + KF_NBMAX * KF_NBMAX;
constexpr int KF_B_K1 = KF_B_K0 + KF_NBMAX;
constexpr int KF_ACC_BLOCKS = KF_B_K1 + KF_NBMAX;
constexpr int KF_ACC_DOUBLES = KF_ACC_BLOCKS * 256;

__device__ __forceinline__ double kf_mfma(double a, double b, double c) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0); }
// one 16 x 16 x 4 product: c[0..3] (rows 4 r + l / 16 of a 16-row block, point / column l % 16) += A(row l % 16, k l / 16) . B(k l / 16, column l % 16).
// Since round 4 the point kernels issue this form (zigp_gemm.h has the story): one A value per lane and product instead of four.
__device__ __forceinline__ void kf_mfma16(double* c, double a, double b) {
  mfma_d4 v = {c[0], c[1], c[2], c[3]};
  v = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, v, 0, 0, 0);
  c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
}

// order LDS traffic of ONE wave: the stores above must be visible to (and not sink below) the loads that follow
__device__ __forceinline__ void kf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// out[4 rb + r] += sum_ks F(rb, ks)[r] * in[ks]:   out (16 nba rows) = A (16 nba x 4 ksn) . in (4 ksn rows), A in fragment order.
// k-steps go in chunks of four, double-buffered by hand: the four fragment loads of chunk c + 1 are issued, a compiler barrier pins
// them there, then come the 16 MFMAs of chunk c.  Left alone the compiler either waits for every load right before its MFMAs (runtime
// bounds: one LDS round trip per k-step) or hoists all loads of the tile (compile-time bounds: hundreds of live registers, spills).
template <int NBA, int QK>
__device__ __forceinline__ void kf_frag_mm(double (&out)[4 * NBA], const double* __restrict__ F, int nba, int ksn, const double (&in)[QK], int lane) {
  static_assert(QK % 4 == 0, "k-steps come in multiples of four (16-row blocks)");
#pragma unroll
  for (int rb = 0; rb < NBA; ++rb) {
    if (rb < nba) {
      const double* __restrict__ Fr = F + rb * ksn * 64 + lane;      // fragment order: one value per lane and (row block, k-step)
      double cur[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = Fr[u * 64];
#pragma unroll
      for (int kc = 0; kc < QK / 4; ++kc) {
        if (4 * kc < ksn) {
          double nxt[4];
          if (4 * (kc + 1) < ksn && kc + 1 < QK / 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) nxt[u] = Fr[(4 * (kc + 1) + u) * 64];
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) nxt[u] = cur[u];
          }
          asm volatile("" ::: "memory");
#pragma unroll
          for (int u = 0; u < 4; ++u) kf_mfma16(&out[4 * rb], cur[u], in[4 * kc + u]);
#pragma unroll
          for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
      }
    }
  }
}

// exp(y) of B values at once, y <= 0.  These are the steps of the device library's exp (same constants, same operations in the same
// order: the results are bit-identical to exp()), written ACROSS the values: sixteen calls of exp() in a row compile to sixteen
// chains of ~16 dependent fp64 operations, one after the other (the kernels around this are at their register limit and the scheduler
// orders for pressure).  Measured with in-kernel stamps on the two K tiles of a 32 x 32 grid: 8.0 k -> 7.3 k cycles from this alone
// (a dependent v_fma_f64 issues every ~5 cycles, so the chains cost less than they look); the branches below were the larger part.
template <int B>
__device__ __forceinline__ void kf_exp_neg(double (&y)[B]) {
  const double LOG2E = __longlong_as_double(0x3ff71547652b82feLL);
  const double NLN2_HI = __longlong_as_double(0xbfe62e42fefa39efLL), NLN2_LO = __longlong_as_double(0xbc7abc9e3b39803fLL);
  const double C11 = __longlong_as_double(0x3e5ade156a5dcb37LL), C10 = __longlong_as_double(0x3e928af3fca7ab0cLL);
  const double CJ[8] = {__longlong_as_double(0x3ec71dee623fde64LL), __longlong_as_double(0x3efa01997c89e6b0LL), __longlong_as_double(0x3f2a01a014761f6eLL),
                        __longlong_as_double(0x3f56c16c1852b7b0LL), __longlong_as_double(0x3f81111111122322LL), __longlong_as_double(0x3fa55555555502a1LL),
                        __longlong_as_double(0x3fc5555555555511LL), __longlong_as_double(0x3fe000000000000bLL)};
  double k[B], r[B], p[B];
#pragma unroll
  for (int i = 0; i < B; ++i) k[i] = __builtin_rint(y[i] * LOG2E);
#pragma unroll
  for (int i = 0; i < B; ++i) r[i] = fma(NLN2_HI, k[i], y[i]);
#pragma unroll
  for (int i = 0; i < B; ++i) r[i] = fma(NLN2_LO, k[i], r[i]);
#pragma unroll
  for (int i = 0; i < B; ++i) p[i] = fma(C11, r[i], C10);
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int i = 0; i < B; ++i) p[i] = fma(r[i], p[i], CJ[j]);
#pragma unroll
  for (int i = 0; i < B; ++i) p[i] = fma(r[i], p[i], 1.0);
#pragma unroll
  for (int i = 0; i < B; ++i) p[i] = fma(r[i], p[i], 1.0);
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const double e = ldexp(p[i], (int)k[i]);
    y[i] = !(-1075.0 > y[i]) ? e : 0.0;      // below: 2^k is out of range of the conversion; exp underflows long before
  }
}

// -0.5 |z_m / ell - x / ell|^2 for the B rows m = 4 (q0 + i) + g of a batch; DD: the input dimension at compile time, 0: runtime f.D
template <int DD, int B>
__device__ __forceinline__ void kf_r2_batch(double (&y)[B], const KfFac& f, const double* zs, const double (&xs)[MAXD], int q0, int g, int mlast) {
  const int D = DD ? DD : f.D;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const int m = min(4 * (q0 + i) + g, mlast);
    double r2 = 0.0;
#pragma unroll
    for (int d = 0; d < (DD ? DD : MAXD); ++d)
      if (d < D) { const double t = zs[m * D + d] - xs[d]; r2 = fma(t, t, r2); }
    y[i] = -0.5 * r2;
  }
}
// K_p tile of this wave: K[q] = k_p(z_{4q+g}, x_n) for the lane's point n, 0 for padding rows / points   (kern.K(Z_p, xnew), :199-201).
// zs = Z_p / ell (LDS copy in the small-grid kernels).  The per-lane conditions (padding row, padding point) are SELECTS, not
// branches: with a branch around each row the 16 loads of z and the 16 exp calls of a tile ran one after the other, each behind
// its own memory round trip (in-kernel stamps: 21 k cycles for a forward tile whose MFMAs take 4.4 k).
// The input dimension of a factor is a kernel argument (wave-uniform).  With `if (d < f.D)` around every term the compiler emits a
// scalar branch per (row, dimension) and waits for each LDS read of z behind its own branch -- 140 branches and 32 serialized LDS
// round trips per pair of K tiles, more than half of the 8.0 k cycles the stamps showed.  SPEC: ONE switch per batch of 8 rows picks a
// straight-line body for D = 1, 2, 3 (the reference's factors are space (2) x time (1), scripts/onoff.py:52-53); larger D loops.
// The kernels with runtime block counts keep the loop form (!SPEC): they are at the register limit and the switch made them spill.
template <int Q, bool SPEC>
__device__ __forceinline__ void kf_ktile(double (&K)[Q], const KfFac& f, int nb, const double* zs, const double* __restrict__ xrow, bool valid, int g) {
  double xs[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) xs[d] = 0.0;
  const auto inv_ell = KF_CONST(f.hyp) + KH_INV;
  const double var = KF_CONST(f.hyp)[KH_VAR];
  if (SPEC && f.D == 1) xs[0] = xrow[f.col0] * inv_ell[0];
  else if (SPEC && f.D == 2) { xs[0] = xrow[f.col0] * inv_ell[0]; xs[1] = xrow[f.col0 + 1] * inv_ell[1]; }
  else {
#pragma unroll
    for (int d = 0; d < MAXD; ++d) xs[d] = (d < f.D) ? xrow[f.col0 + d] * inv_ell[d] : 0.0;
  }
  constexpr int B = Q < 8 ? Q : 8;
  const int mlast = 16 * nb - 1;             // zs holds 16 nb rows: blocks beyond nb (runtime block counts) read its last row and are zeroed below
#pragma unroll
  for (int q0 = 0; q0 < Q; q0 += B) {
    double y[B];
    if (SPEC) {
      switch (f.D) {
        case 1: kf_r2_batch<1, B>(y, f, zs, xs, q0, g, mlast); break;
        case 2: kf_r2_batch<2, B>(y, f, zs, xs, q0, g, mlast); break;
        case 3: kf_r2_batch<3, B>(y, f, zs, xs, q0, g, mlast); break;
        default: kf_r2_batch<0, B>(y, f, zs, xs, q0, g, mlast);
      }
    } else {
      kf_r2_batch<0, B>(y, f, zs, xs, q0, g, mlast);
    }
    kf_exp_neg<B>(y);
#pragma unroll
    for (int i = 0; i < B; ++i)
      if (q0 + i < Q) {
        const int m = 4 * (q0 + i) + g;
        K[q0 + i] = (m < f.M && m <= mlast && valid) ? var * y[i] : 0.0;
      }
  }
}

// ---- Matern factors on the fused path (zigp_set_kron_matern_fused): the _kinds kernels ----------------------------------------------
// The kernels whose names end in _kinds stand beside the RBF kernels and are launched only for a call that has a Matern factor.  Each
// follows the RBF kernel it was taken from, as a *_kinds_body function, and is that kernel's text with the Matern pieces added.  The text
// is kept twice on purpose: with the RBF kernels routed through a shared body (a template flag) they compiled to the same instruction
// counts under another register allocation, and their machine code is pinned (tools/isa_compare.py).  A fix to an RBF point kernel has
// to be made in its _kinds_body as well.  The _kinds kernels take one more argument, the kinds of the call's
// four factors packed two bits each (bit 2 (2 h + q): ZIGP_KERN_* of factor q of latent h), so no argument of an RBF kernel moves; the
// kind of a factor is wave-uniform and read at run time.
__host__ __device__ inline int kf_kind_of(int kinds, int h, int q) { return (kinds >> (2 * (2 * h + q))) & 3; }

// kf_ktile for a factor of any kind; GRAD also gives Kd = K' = -dk / d(r2 / 2) (K' = K for RBF).  r2 is formed by kf_r2_batch exactly as
// for RBF (y = -r2 / 2, so -2 y is r2 again, exactly), then kron_matern_elem's arithmetic (zigp_kron.hip): r = sqrt(min(r2, 2^996) + 1e-12),
// t = sqrt3 r or sqrt5 r, e = exp(-t) through kf_exp_neg, K = var (1 + t) e or var (1 + t + 5/3 r^2) e.  A far pair gives a finite
// polynomial times e = +0.  An RBF factor takes kf_ktile itself: the same bits as in the RBF instantiation.
template <int Q, bool SPEC, bool GRAD>
__device__ __forceinline__ void kf_ktile_kinds(double (&K)[Q], double (&Kd)[Q], int kind, const KfFac& f, int nb, const double* zs,
                                               const double* __restrict__ xrow, bool valid, int g) {
  if (kind == KERN_RBF) {
    kf_ktile<Q, SPEC>(K, f, nb, zs, xrow, valid, g);
    if (GRAD) {
#pragma unroll
      for (int q = 0; q < Q; ++q) Kd[q] = K[q];
    }
    return;
  }
  double xs[MAXD];
  const auto inv_ell = KF_CONST(f.hyp) + KH_INV;
  const double var = KF_CONST(f.hyp)[KH_VAR];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) xs[d] = (d < f.D) ? xrow[f.col0 + d] * inv_ell[d] : 0.0;
  const bool m32 = kind == KERN_M32;
  const double ca = m32 ? MATERN_SQRT3 : MATERN_SQRT5;
  constexpr int B = Q < 8 ? Q : 8;
  const int mlast = 16 * nb - 1;
#pragma unroll
  for (int q0 = 0; q0 < Q; q0 += B) {
    double y[B], r[B], tt[B];
    if (SPEC) {
      switch (f.D) {
        case 1: kf_r2_batch<1, B>(y, f, zs, xs, q0, g, mlast); break;
        case 2: kf_r2_batch<2, B>(y, f, zs, xs, q0, g, mlast); break;
        case 3: kf_r2_batch<3, B>(y, f, zs, xs, q0, g, mlast); break;
        default: kf_r2_batch<0, B>(y, f, zs, xs, q0, g, mlast);
      }
    } else {
      kf_r2_batch<0, B>(y, f, zs, xs, q0, g, mlast);
    }
#pragma unroll
    for (int i = 0; i < B; ++i) {
      r[i] = sqrt(fmin(-2.0 * y[i], 0x1p+996) + MATERN_FLOOR);
      tt[i] = ca * r[i];
      y[i] = -tt[i];
    }
    kf_exp_neg<B>(y);
#pragma unroll
    for (int i = 0; i < B; ++i)
      if (q0 + i < Q) {
        const int m = 4 * (q0 + i) + g;
        const bool on = m < f.M && m <= mlast && valid;
        const double p1 = 1.0 + tt[i];
        const double poly = m32 ? p1 : p1 + (5.0 / 3.0) * (r[i] * r[i]);
        K[q0 + i] = on ? var * poly * y[i] : 0.0;
        if (GRAD) Kd[q0 + i] = on ? (m32 ? 3.0 * var * y[i] : (5.0 / 3.0) * var * p1 * y[i]) : 0.0;
      }
  }
}

// sum over the 4 row groups (lanes l, l^16, l^32, l^48): every lane ends with the column total, fixed order
__device__ __forceinline__ double kf_colsum(double v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

constexpr int KF_Q = 4 * KF_NBMAX;   // registers per [16 nb][16] tile quantity
constexpr int KF_MQ_ = 16 * KF_NBMAX;

// The workgroup's copy of the fragment images in LDS (8 KB each at 32 x 32): every wave re-reads them for every tile, and an LDS
// read returns in ~100 cycles where an L2 hit takes 500+ (one wave per SIMD has nothing else to hide that behind).
constexpr int KF_FRAG = KF_MQ_ * KF_MQ_;
struct KfFrags { const double *P0, *P1, *Al, *S2, *AlT, *S2T; const double *Z0, *Z1; };   // + the scaled inducing inputs
__device__ __forceinline__ void kf_stage_z(double* dst, const KfFac& f) {
  for (int idx = threadIdx.x; idx < 16 * f.nb * f.D; idx += blockDim.x) dst[idx] = f.Zs[idx];
}
// n is a multiple of 256.  32 bytes per lane and load, eight loads in flight per thread: the larger grids stage 130-160 KB per
// workgroup (P1 alone is 100 KB at 100 points), and with 16-byte loads four at a time the copy was a chain of ~20 L2 round trips in
// front of a workgroup's only tile (minibatch steps: one tile per wave).
__device__ __forceinline__ void kf_stage_frag(double* dst, const double* __restrict__ src, int n) {
  const double4* __restrict__ s4 = reinterpret_cast<const double4*>(src);
  double4* d4 = reinterpret_cast<double4*>(dst);
  const int n4 = n / 4, step = blockDim.x;
  int idx = threadIdx.x;
  for (; idx + 7 * step < n4; idx += 8 * step) {
    double4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = s4[idx + u * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) d4[idx + u * step] = v[u];
  }
  for (; idx < n4; idx += step) d4[idx] = s4[idx];
}

// The same copy without registers: global_load_lds moves 1 KB per wave instruction straight into LDS and only counts on vmcnt, so a
// kernel can issue the whole image, compute what does not need it (the K tiles of its first tile), and wait in kf_stage_wait().
// n is a multiple of 256 doubles (2 KB): chunk c = 128 doubles, dealt out over the waves of the workgroup.
__device__ __forceinline__ void kf_stage_frag_async(double* dst, const double* __restrict__ src, int n) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6, lane = threadIdx.x & 63;
  for (int c = wave; c < n / 128; c += nwaves)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (int64_t)c * 128 + 2 * lane),
                                     (__attribute__((address_space(3))) void*)(dst + c * 128), 16, 0, 0);
}
__device__ __forceinline__ void kf_stage_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Per-tile state of one latent for a grid of NB0 x NB1 16-row blocks.  EXACT kernels are instantiated for the block counts they run
// with: every loop bound is then a compile-time constant, the guards fold away and the compiler issues the fragment loads of a
// product ahead of its MFMAs.  With runtime bounds each 16 x 16 x 4 step sat behind its own LDS round trip (in-kernel stamps: 21 k
// cycles for the 64 products of a forward tile whose MFMAs take 4.4 k).
template <int NB0, int NB1> struct KfTile { double K0[4 * NB0], K1[4 * NB1], A0[4 * NB0], A1[4 * NB1], B0[4 * NB0], C0[4 * NB0]; };

// forward pieces of one tile: the K tiles (need the inducing inputs only), then A_p = P_p K_p, B0 = Alpha K1, C0 = S2 A1^2 (fragment images)
template <int NB0, int NB1, bool EXACT>
__device__ __forceinline__ void kf_forward_ktiles(KfTile<NB0, NB1>& t, const KfLat& L, const double* Z0, const double* Z1, const double* __restrict__ xrow,
                                                  bool valid, int g) {
  const KfFac &f0 = L.f[0], &f1 = L.f[1];
  const int nb0 = EXACT ? NB0 : f0.nb, nb1 = EXACT ? NB1 : f1.nb;
  kf_ktile<4 * NB0, EXACT>(t.K0, f0, nb0, Z0, xrow, valid, g);
  kf_ktile<4 * NB1, EXACT>(t.K1, f1, nb1, Z1, xrow, valid, g);
}
// kf_forward_ktiles for factors of any kind: lk = kind0 + 4 kind1 of this latent; GRAD: also the K' tiles
template <int NB0, int NB1, bool EXACT, bool GRAD>
__device__ __forceinline__ void kf_ktiles_any(KfTile<NB0, NB1>& t, double (&Kd0)[4 * NB0], double (&Kd1)[4 * NB1], int lk, const KfLat& L, const double* Z0,
                                              const double* Z1, const double* __restrict__ xrow, bool valid, int g) {
  const KfFac &f0 = L.f[0], &f1 = L.f[1];
  const int nb0 = EXACT ? NB0 : f0.nb, nb1 = EXACT ? NB1 : f1.nb;
  kf_ktile_kinds<4 * NB0, EXACT, GRAD>(t.K0, Kd0, lk & 3, f0, nb0, Z0, xrow, valid, g);
  kf_ktile_kinds<4 * NB1, EXACT, GRAD>(t.K1, Kd1, lk >> 2, f1, nb1, Z1, xrow, valid, g);
}
template <int NB0, int NB1, bool EXACT>
__device__ __forceinline__ void kf_forward_products(KfTile<NB0, NB1>& t, const KfLat& L, const KfFrags& F, int slot) {
  const int nb0 = EXACT ? NB0 : L.f[0].nb, nb1 = EXACT ? NB1 : L.f[1].nb;
#pragma unroll
  for (int q = 0; q < 4 * NB0; ++q) { t.A0[q] = 0.0; t.B0[q] = 0.0; t.C0[q] = 0.0; }
#pragma unroll
  for (int q = 0; q < 4 * NB1; ++q) t.A1[q] = 0.0;
  kf_frag_mm<NB0, 4 * NB0>(t.A0, F.P0, nb0, 4 * nb0, t.K0, slot);
  kf_frag_mm<NB1, 4 * NB1>(t.A1, F.P1, nb1, 4 * nb1, t.K1, slot);
  kf_frag_mm<NB0, 4 * NB1>(t.B0, F.Al, nb0, 4 * nb1, t.K1, slot);
  double sq[4 * NB1];
#pragma unroll
  for (int q = 0; q < 4 * NB1; ++q) sq[q] = t.A1[q] * t.A1[q];
  kf_frag_mm<NB0, 4 * NB1>(t.C0, F.S2, nb0, 4 * nb1, sq, slot);
}
template <int NB0, int NB1, bool EXACT>
__device__ __forceinline__ void kf_forward_tile(KfTile<NB0, NB1>& t, const KfLat& L, const KfFrags& F, const double* __restrict__ xrow, bool valid,
                                                int g, int slot) {
  kf_forward_ktiles<NB0, NB1, EXACT>(t, L, F.Z0, F.Z1, xrow, valid, g);
  kf_forward_products<NB0, NB1, EXACT>(t, L, F, slot);
}

// ---- forward: part[0..3][n] = q0 = k0.a0, q1 = k1.a1, mean = k0^T Alpha k1, st = (a0^2)^T S2 (a1^2) -------------------------
template <int NB0, int NB1>
__global__ void __launch_bounds__(64 * KF_WAVES)
k_kf_forward(KfArgs a) {
  __shared__ double sfr[4 * KF_FRAG];
  __shared__ double sz[2][KF_MQ_ * MAXD];
  const KfLat& L = a.lat[a.lat0 + blockIdx.y];
  {
    constexpr int n0 = NB0 * NB0 * 256, n1 = NB1 * NB1 * 256, n01 = NB0 * NB1 * 256;
    // asynchronous copies (kf_stage_frag_async): the K tiles of the wave's first tile are computed underneath them, from the global
    // copy of the scaled inducing inputs (the LDS copy becomes visible with the images, at kf_stage_wait)
    kf_stage_frag_async(sfr, L.f[0].PF, n0); kf_stage_frag_async(sfr + KF_FRAG, L.f[1].PF, n1);
    kf_stage_frag_async(sfr + 2 * KF_FRAG, L.AlF, n01); kf_stage_frag_async(sfr + 3 * KF_FRAG, L.S2F, n01);
    kf_stage_z(sz[0], L.f[0]); kf_stage_z(sz[1], L.f[1]);
  }
  const KfFrags F = {sfr, sfr + KF_FRAG, sfr + 2 * KF_FRAG, sfr + 3 * KF_FRAG, nullptr, nullptr, sz[0], sz[1]};
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15, slot = lane;      // slot: this lane's position in a fragment block
  const int w = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);
  const int t1 = min((w + 1) * a.tpw, a.ntiles);
  KfTile<NB0, NB1> t;
  bool first = true;
  if (w * a.tpw < t1) {
    const int64_t pn = (int64_t)(w * a.tpw) * 16 + n;
    kf_forward_ktiles<NB0, NB1, true>(t, L, L.f[0].Zs, L.f[1].Zs, a.X + (pn < a.N ? pn : 0) * a.ldx, pn < a.N, g);
  }
  kf_stage_wait();
  for (int tile = w * a.tpw; tile < t1; ++tile) {
    const int64_t pn = (int64_t)tile * 16 + n;
    const bool valid = pn < a.N;
    if (!first) kf_forward_ktiles<NB0, NB1, true>(t, L, F.Z0, F.Z1, a.X + (valid ? pn : 0) * a.ldx, valid, g);
    first = false;
    kf_forward_products<NB0, NB1, true>(t, L, F, slot);
    double q0 = 0.0, q1 = 0.0, mu = 0.0, st = 0.0;
#pragma unroll
    for (int q = 0; q < 4 * NB0; ++q) {
      q0 = fma(t.K0[q], t.A0[q], q0);
      mu = fma(t.K0[q], t.B0[q], mu);
      st = fma(t.A0[q] * t.A0[q], t.C0[q], st);
    }
#pragma unroll
    for (int q = 0; q < 4 * NB1; ++q) q1 = fma(t.K1[q], t.A1[q], q1);
    q0 = kf_colsum(q0); q1 = kf_colsum(q1); mu = kf_colsum(mu); st = kf_colsum(st);
    if (g == 0) { L.part[pn] = q0; L.part[a.Npad + pn] = q1; L.part[2 * a.Npad + pn] = mu; L.part[3 * a.Npad + pn] = st; }
  }
}
template <int NB0, int NB1>
__device__ __forceinline__ void kf_forward_kinds_body(const KfArgs& a, int kinds, double* sfr, double (*sz)[KF_MQ_ * MAXD]) {
  const KfLat& L = a.lat[a.lat0 + blockIdx.y];
  const int lk = (kinds >> (4 * (a.lat0 + blockIdx.y))) & 15;
  double kd0[4 * NB0], kd1[4 * NB1];      // K' is not needed going forward (GRAD = false leaves them unwritten)
  {
    constexpr int n0 = NB0 * NB0 * 256, n1 = NB1 * NB1 * 256, n01 = NB0 * NB1 * 256;
    // asynchronous copies (kf_stage_frag_async): the K tiles of the wave's first tile are computed underneath them, from the global
    // copy of the scaled inducing inputs (the LDS copy becomes visible with the images, at kf_stage_wait)
    kf_stage_frag_async(sfr, L.f[0].PF, n0); kf_stage_frag_async(sfr + KF_FRAG, L.f[1].PF, n1);
    kf_stage_frag_async(sfr + 2 * KF_FRAG, L.AlF, n01); kf_stage_frag_async(sfr + 3 * KF_FRAG, L.S2F, n01);
    kf_stage_z(sz[0], L.f[0]); kf_stage_z(sz[1], L.f[1]);
  }
  const KfFrags F = {sfr, sfr + KF_FRAG, sfr + 2 * KF_FRAG, sfr + 3 * KF_FRAG, nullptr, nullptr, sz[0], sz[1]};
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15, slot = lane;      // slot: this lane's position in a fragment block
  const int w = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);
  const int t1 = min((w + 1) * a.tpw, a.ntiles);
  KfTile<NB0, NB1> t;
  bool first = true;
  if (w * a.tpw < t1) {
    const int64_t pn = (int64_t)(w * a.tpw) * 16 + n;
    kf_ktiles_any<NB0, NB1, true, false>(t, kd0, kd1, lk, L, L.f[0].Zs, L.f[1].Zs, a.X + (pn < a.N ? pn : 0) * a.ldx, pn < a.N, g);
  }
  kf_stage_wait();
  for (int tile = w * a.tpw; tile < t1; ++tile) {
    const int64_t pn = (int64_t)tile * 16 + n;
    const bool valid = pn < a.N;
    if (!first) kf_ktiles_any<NB0, NB1, true, false>(t, kd0, kd1, lk, L, F.Z0, F.Z1, a.X + (valid ? pn : 0) * a.ldx, valid, g);
    first = false;
    kf_forward_products<NB0, NB1, true>(t, L, F, slot);
    double q0 = 0.0, q1 = 0.0, mu = 0.0, st = 0.0;
#pragma unroll
    for (int q = 0; q < 4 * NB0; ++q) {
      q0 = fma(t.K0[q], t.A0[q], q0);
      mu = fma(t.K0[q], t.B0[q], mu);
      st = fma(t.A0[q] * t.A0[q], t.C0[q], st);
    }
#pragma unroll
    for (int q = 0; q < 4 * NB1; ++q) q1 = fma(t.K1[q], t.A1[q], q1);
    q0 = kf_colsum(q0); q1 = kf_colsum(q1); mu = kf_colsum(mu); st = kf_colsum(st);
    if (g == 0) { L.part[pn] = q0; L.part[a.Npad + pn] = q1; L.part[2 * a.Npad + pn] = mu; L.part[3 * a.Npad + pn] = st; }
  }
}
template <int NB0, int NB1>
__global__ void __launch_bounds__(64 * KF_WAVES)
k_kf_forward_kinds(KfArgs a, int kinds) {
  __shared__ double sfr[4 * KF_FRAG];
  __shared__ double sz[2][KF_MQ_ * MAXD];
  kf_forward_kinds_body<NB0, NB1>(a, kinds, sfr, sz);
}

// tile in registers -> LDS image [row][KF_LD]
template <int Q>
__device__ __forceinline__ void kf_store_tile(double* T, const double (&V)[Q], int g, int n) {
#pragma unroll
  for (int q = 0; q < Q; ++q) T[(4 * q + g) * KF_LD + n] = V[q];
}
// acc[(rb, cb)] += A(rows of rb, 16 points) . B(16 points, cols of cb), A / B from LDS tiles (rows x points), optional squares and
// per-point scale on B;  MODE 0: plain, 1: both squared
template <int NBR, int NBC, int MODE, bool SCALED>
__device__ __forceinline__ void kf_accum(double (&acc)[NBR * NBC][4], const double* TA, const double* TB, const double (&sck)[4], int lane) {
  const int kk = lane >> 4, bj = lane & 15;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    double bf[NBC];
#pragma unroll
    for (int cb = 0; cb < NBC; ++cb) {
      double b = TB[(16 * cb + bj) * KF_LD + 4 * ks + kk];
      if (MODE == 1) b *= b;
      if (SCALED) b *= sck[ks];
      bf[cb] = b;
    }
#pragma unroll
    for (int rb = 0; rb < NBR; ++rb) {
      double v = TA[(16 * rb + bj) * KF_LD + 4 * ks + kk];      // A operand: (row l % 16, point 4 ks + l / 16)
      if (MODE == 1) v *= v;
#pragma unroll
      for (int cb = 0; cb < NBC; ++cb) kf_mfma16(acc[rb * NBC + cb], v, bf[cb]);
    }
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// per point, with gm / gv the cotangents of mean / var and dq_p = -gv q_other:
//   B1 = Alpha^T K0, C1 = S2^T A0^2 ;  dA_p = 2 gv A_p . C_p ;  dK_p = gm B_p + 2 dq_p A_p + P_p dA_p ;  E_p = dq_p K_p + dA_p
//   dAlpha += K0 diag(gm) K1^T ; dS2 += A0^2 diag(gv) (A1^2)^T ; dP_p += E_p K_p^T
//   moments of t_p = dK_p . K_p against {1, x - zc, (x - zc)^2}  (-> d var_p, d Z_p, d ell_p in k_kf_finish)
template <int NB0, int NB1>
__global__ void __launch_bounds__(64 * KF_WAVES, 1)
k_kf_backward(KfArgs a) {
  extern __shared__ double lds[];
  const KfLat& L = a.lat[a.lat0 + blockIdx.y];
  const KfFac &f0 = L.f[0], &f1 = L.f[1];
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15, slot = lane;      // slot: this lane's position in a fragment block
  const int wib = threadIdx.x >> 6;
  const int w = blockIdx.x * KF_WAVES + wib;
  constexpr int Q0 = 4 * NB0, Q1 = 4 * NB1;
  constexpr int TILE = 16 * KF_NBMAX * KF_LD;
  double* bK0 = lds + wib * 4 * TILE; double* bK1 = bK0 + TILE; double* c0 = bK1 + TILE; double* c1 = c0 + TILE;
  double* sfr = lds + KF_WAVES * 4 * TILE;
  {
    constexpr int n0 = NB0 * NB0 * 256, n1 = NB1 * NB1 * 256, n01 = NB0 * NB1 * 256;
    kf_stage_frag_async(sfr, f0.PF, n0); kf_stage_frag_async(sfr + KF_FRAG, f1.PF, n1);
    kf_stage_frag_async(sfr + 2 * KF_FRAG, L.AlF, n01); kf_stage_frag_async(sfr + 3 * KF_FRAG, L.S2F, n01);
    kf_stage_frag_async(sfr + 4 * KF_FRAG, L.AlTF, n01); kf_stage_frag_async(sfr + 5 * KF_FRAG, L.S2TF, n01);
    kf_stage_z(sfr + 6 * KF_FRAG, f0); kf_stage_z(sfr + 6 * KF_FRAG + KF_MQ_ * MAXD, f1);
  }
  const KfFrags F = {sfr, sfr + KF_FRAG, sfr + 2 * KF_FRAG, sfr + 3 * KF_FRAG, sfr + 4 * KF_FRAG, sfr + 5 * KF_FRAG,
                     sfr + 6 * KF_FRAG, sfr + 6 * KF_FRAG + KF_MQ_ * MAXD};
  double accAl[NB0 * NB1][4], accS2[NB0 * NB1][4], accP0[NB0 * NB0][4], accP1[NB1 * NB1][4], accK0[NB0][4], accK1[NB1][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int b = 0; b < NB0 * NB1; ++b) { accAl[b][r] = 0.0; accS2[b][r] = 0.0; }
#pragma unroll
    for (int b = 0; b < NB0 * NB0; ++b) accP0[b][r] = 0.0;
#pragma unroll
    for (int b = 0; b < NB1 * NB1; ++b) accP1[b][r] = 0.0;
#pragma unroll
    for (int b = 0; b < NB0; ++b) accK0[b][r] = 0.0;
#pragma unroll
    for (int b = 0; b < NB1; ++b) accK1[b][r] = 0.0;
  }
  const double one4[4] = {1.0, 1.0, 1.0, 1.0};
  // column j = n of the moment matrix Psi_p: 0 -> 1, 1..D -> x_d - zc_d, D+1..2D -> (x_d - zc_d)^2, beyond -> 0   (fixed per lane)
  int psi_kind[2], psi_col[2]; double psi_zc[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const KfFac& f = L.f[p];
    const int d = (n == 0) ? 0 : ((n <= f.D) ? n - 1 : ((n <= 2 * f.D) ? n - 1 - f.D : 0));
    psi_kind[p] = (n == 0) ? 0 : ((n <= f.D) ? 1 : ((n <= 2 * f.D) ? 2 : 3));
    psi_col[p] = f.col0 + d; psi_zc[p] = KF_CONST(f.hyp)[KH_ZC + d];
  }

  const int t1 = min((w + 1) * a.tpw, a.ntiles);
  KfTile<NB0, NB1> t;
  bool first = true;
  if (w * a.tpw < t1) {          // K tiles of the first tile under the asynchronous staging copies (global copy of the inducing inputs)
    const int64_t pn = (int64_t)(w * a.tpw) * 16 + n;
    kf_forward_ktiles<NB0, NB1, true>(t, L, f0.Zs, f1.Zs, a.X + (pn < a.N ? pn : 0) * a.ldx, pn < a.N, g);
  }
  kf_stage_wait();
  for (int tile = w * a.tpw; tile < t1; ++tile) {
    const int64_t pn = (int64_t)tile * 16 + n;
    const bool valid = pn < a.N;
    const double* xrow = a.X + (valid ? pn : 0) * a.ldx;
    if (!first) kf_forward_ktiles<NB0, NB1, true>(t, L, F.Z0, F.Z1, xrow, valid, g);
    first = false;
    kf_forward_products<NB0, NB1, true>(t, L, F, slot);
    const double gmn = L.gm[pn], gvn = L.gv[pn], dq0n = L.dq0[pn], dq1n = L.dq1[pn];   // zero for padding points (scale 0 in the point-wise kernel)
    double B1[Q1], C1[Q1], sq[Q0];
#pragma unroll
    for (int q = 0; q < Q1; ++q) { B1[q] = 0.0; C1[q] = 0.0; }
#pragma unroll
    for (int q = 0; q < Q0; ++q) sq[q] = t.A0[q] * t.A0[q];
    kf_frag_mm<NB1, Q0>(B1, F.AlT, NB1, Q0, t.K0, slot);
    kf_frag_mm<NB1, Q0>(C1, F.S2T, NB1, Q0, sq, slot);
    double dA0[Q0], dA1[Q1], PdA0[Q0], PdA1[Q1];
#pragma unroll
    for (int q = 0; q < Q0; ++q) { dA0[q] = 2.0 * gvn * t.A0[q] * t.C0[q]; PdA0[q] = 0.0; }
#pragma unroll
    for (int q = 0; q < Q1; ++q) { dA1[q] = 2.0 * gvn * t.A1[q] * C1[q]; PdA1[q] = 0.0; }
    kf_frag_mm<NB0, Q0>(PdA0, F.P0, NB0, Q0, dA0, slot);
    kf_frag_mm<NB1, Q1>(PdA1, F.P1, NB1, Q1, dA1, slot);
    // ---- LDS images for the sums over points (k index = point): K tiles, E tiles
    kf_store_tile<Q0>(bK0, t.K0, g, n);
    kf_store_tile<Q1>(bK1, t.K1, g, n);
    {
      double E0[Q0], E1[Q1];
#pragma unroll
      for (int q = 0; q < Q0; ++q) E0[q] = fma(dq0n, t.K0[q], dA0[q]);
      kf_store_tile<Q0>(c0, E0, g, n);
#pragma unroll
      for (int q = 0; q < Q1; ++q) E1[q] = fma(dq1n, t.K1[q], dA1[q]);
      kf_store_tile<Q1>(c1, E1, g, n);
    }
    kf_wave_sync();
    double gmk[4], gvk[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { gmk[ks] = __shfl(gmn, 4 * ks + g, 64); gvk[ks] = __shfl(gvn, 4 * ks + g, 64); }
    kf_accum<NB0, NB1, 0, true>(accAl, bK0, bK1, gmk, lane);
    kf_accum<NB0, NB0, 0, false>(accP0, c0, bK0, one4, lane);
    kf_accum<NB1, NB1, 0, false>(accP1, c1, bK1, one4, lane);
    kf_wave_sync();
    // B operand of the moment products: lane (kk = g, column j = n) needs psi_j of point 4 ks + g -- loaded here (most of the tile state
    // is dead by now), the round trip hides behind the dS2 products
    double psi[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        // selects, not branches: the eight loads go out back to back (one round trip, not eight)
        const int64_t pt = (int64_t)tile * 16 + 4 * ks + g;
        const double xv = a.X[(pt < a.N ? pt : 0) * a.ldx + psi_col[p]] - psi_zc[p];
        const double v = psi_kind[p] == 0 ? 1.0 : (psi_kind[p] == 1 ? xv : (psi_kind[p] == 2 ? xv * xv : 0.0));
        psi[p][ks] = (pt < a.N) ? v : 0.0;
      }
    kf_store_tile<Q0>(c0, t.A0, g, n);
    kf_store_tile<Q1>(c1, t.A1, g, n);
    kf_wave_sync();
    kf_accum<NB0, NB1, 1, true>(accS2, c0, c1, gvk, lane);
    kf_wave_sync();
    {
      double t0[Q0], t1v[Q1];
#pragma unroll
      for (int q = 0; q < Q0; ++q) t0[q] = fma(gmn, t.B0[q], fma(2.0 * dq0n, t.A0[q], PdA0[q])) * t.K0[q];
      kf_store_tile<Q0>(c0, t0, g, n);
#pragma unroll
      for (int q = 0; q < Q1; ++q) t1v[q] = fma(gmn, B1[q], fma(2.0 * dq1n, t.A1[q], PdA1[q])) * t.K1[q];
      kf_store_tile<Q1>(c1, t1v, g, n);
    }
    kf_wave_sync();
    // moments: acc(rows of factor p, col j) += sum_n t_p[row, n] psi_j(x_n),  psi = {1, xc_d, xc_d^2}
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int rb = 0; rb < NB0; ++rb) kf_mfma16(accK0[rb], c0[(16 * rb + n) * KF_LD + 4 * ks + g], psi[0][ks]);
#pragma unroll
      for (int rb = 0; rb < NB1; ++rb) kf_mfma16(accK1[rb], c1[(16 * rb + n) * KF_LD + 4 * ks + g], psi[1][ks]);
    }
    kf_wave_sync();
  }
  // per-wave partials, [block][r][lane]; blocks numbered for the CAPACITY grid (KF_NBMAX x KF_NBMAX) that k_kf_reduce / k_kf_finish index
  double* out = L.acc + (int64_t)w * KF_ACC_DOUBLES;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int rb = 0; rb < NB0; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB1; ++cb) {
        out[((KF_B_AL + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accAl[rb * NB1 + cb][r];
        out[((KF_B_S2 + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accS2[rb * NB1 + cb][r];
      }
#pragma unroll
    for (int rb = 0; rb < NB0; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB0; ++cb) out[((KF_B_P0 + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accP0[rb * NB0 + cb][r];
#pragma unroll
    for (int rb = 0; rb < NB1; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB1; ++cb) out[((KF_B_P1 + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accP1[rb * NB1 + cb][r];
#pragma unroll
    for (int rb = 0; rb < NB0; ++rb) out[((KF_B_K0 + rb) * 4 + r) * 64 + lane] = accK0[rb][r];
#pragma unroll
    for (int rb = 0; rb < NB1; ++rb) out[((KF_B_K1 + rb) * 4 + r) * 64 + lane] = accK1[rb][r];
  }
}
// k_kf_backward_kinds: the moment columns 1 .. 2 D of a Matern factor take t' = dK . K' in place of t = dK . K (column 0, the
// variance, keeps t).  One MFMA chain has one A operand, so the moments are two chains per factor: t against Psi masked to the columns
// that take K, then t' against Psi masked to the others; a column gets its products from one chain and exact zeros from the other, so an
// RBF factor (every column in the first chain, t' = t) ends with the bits of the RBF instantiation.  The second chain of a Matern factor
// also fills column 15 of its moment block with sum t' (Psi = 1; the column is free, D <= 7 on this path): the finish kernel re-centres
// the t' moments with it, as it re-centres an RBF factor's with column 0.  K' waits in a lane-private LDS image
// written with the K tile (kd[q * 64 + lane], 2 * KF_Q * 64 doubles per wave behind the fragment images): the accumulators and the tile
// state leave no registers for it.
template <int NB0, int NB1>
__device__ __forceinline__ void kf_backward_kinds_body(const KfArgs& a, int kinds, double* lds) {
  const KfLat& L = a.lat[a.lat0 + blockIdx.y];
  const KfFac &f0 = L.f[0], &f1 = L.f[1];
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15, slot = lane;      // slot: this lane's position in a fragment block
  const int wib = threadIdx.x >> 6;
  const int lk = (kinds >> (4 * (a.lat0 + blockIdx.y))) & 15;
  const int w = blockIdx.x * KF_WAVES + wib;
  constexpr int Q0 = 4 * NB0, Q1 = 4 * NB1;
  constexpr int TILE = 16 * KF_NBMAX * KF_LD;
  double* bK0 = lds + wib * 4 * TILE; double* bK1 = bK0 + TILE; double* c0 = bK1 + TILE; double* c1 = c0 + TILE;
  double* sfr = lds + KF_WAVES * 4 * TILE;
  {
    constexpr int n0 = NB0 * NB0 * 256, n1 = NB1 * NB1 * 256, n01 = NB0 * NB1 * 256;
    kf_stage_frag_async(sfr, f0.PF, n0); kf_stage_frag_async(sfr + KF_FRAG, f1.PF, n1);
    kf_stage_frag_async(sfr + 2 * KF_FRAG, L.AlF, n01); kf_stage_frag_async(sfr + 3 * KF_FRAG, L.S2F, n01);
    kf_stage_frag_async(sfr + 4 * KF_FRAG, L.AlTF, n01); kf_stage_frag_async(sfr + 5 * KF_FRAG, L.S2TF, n01);
    kf_stage_z(sfr + 6 * KF_FRAG, f0); kf_stage_z(sfr + 6 * KF_FRAG + KF_MQ_ * MAXD, f1);
  }
  const KfFrags F = {sfr, sfr + KF_FRAG, sfr + 2 * KF_FRAG, sfr + 3 * KF_FRAG, sfr + 4 * KF_FRAG, sfr + 5 * KF_FRAG,
                     sfr + 6 * KF_FRAG, sfr + 6 * KF_FRAG + KF_MQ_ * MAXD};
  double accAl[NB0 * NB1][4], accS2[NB0 * NB1][4], accP0[NB0 * NB0][4], accP1[NB1 * NB1][4], accK0[NB0][4], accK1[NB1][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int b = 0; b < NB0 * NB1; ++b) { accAl[b][r] = 0.0; accS2[b][r] = 0.0; }
#pragma unroll
    for (int b = 0; b < NB0 * NB0; ++b) accP0[b][r] = 0.0;
#pragma unroll
    for (int b = 0; b < NB1 * NB1; ++b) accP1[b][r] = 0.0;
#pragma unroll
    for (int b = 0; b < NB0; ++b) accK0[b][r] = 0.0;
#pragma unroll
    for (int b = 0; b < NB1; ++b) accK1[b][r] = 0.0;
  }
  const double one4[4] = {1.0, 1.0, 1.0, 1.0};
  // column j = n of the moment matrix Psi_p: 0 -> 1, 1..D -> x_d - zc_d, D+1..2D -> (x_d - zc_d)^2, beyond -> 0   (fixed per lane)
  int psi_kind[2], psi_col[2]; double psi_zc[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const KfFac& f = L.f[p];
    const int d = (n == 0) ? 0 : ((n <= f.D) ? n - 1 : ((n <= 2 * f.D) ? n - 1 - f.D : 0));
    psi_kind[p] = (n == 0) ? 0 : ((n <= f.D) ? 1 : ((n <= 2 * f.D) ? 2 : 3));
    // a Matern factor: column 15 (free: D <= 7 on this path) is the constant 1 again, in the SECOND chain -- sum t', which the finish
    // kernel needs to re-centre the t' moments around z_m (column 0 is sum t)
    if (n == 15 && ((lk >> (2 * p)) & 3) != KERN_RBF) psi_kind[p] = 0;
    psi_col[p] = f.col0 + d; psi_zc[p] = KF_CONST(f.hyp)[KH_ZC + d];
  }

  const int t1 = min((w + 1) * a.tpw, a.ntiles);
  KfTile<NB0, NB1> t;
  // this lane's K' values of the tile, factor 0 then factor 1 (written and read by the same lane: no synchronisation)
  double* const kdl = lds + KF_WAVES * 4 * TILE + 6 * KF_FRAG + 2 * KF_MQ_ * MAXD + wib * 2 * KF_Q * 64 + lane;
  bool first = true;
  if (w * a.tpw < t1) {          // K tiles of the first tile under the asynchronous staging copies (global copy of the inducing inputs)
    const int64_t pn = (int64_t)(w * a.tpw) * 16 + n;
    double kd0[Q0], kd1[Q1];
    kf_ktiles_any<NB0, NB1, true, true>(t, kd0, kd1, lk, L, f0.Zs, f1.Zs, a.X + (pn < a.N ? pn : 0) * a.ldx, pn < a.N, g);
    {
#pragma unroll
      for (int q = 0; q < Q0; ++q) kdl[q * 64] = kd0[q];
#pragma unroll
      for (int q = 0; q < Q1; ++q) kdl[(KF_Q + q) * 64] = kd1[q];
    }
  }
  kf_stage_wait();
  for (int tile = w * a.tpw; tile < t1; ++tile) {
    const int64_t pn = (int64_t)tile * 16 + n;
    const bool valid = pn < a.N;
    const double* xrow = a.X + (valid ? pn : 0) * a.ldx;
    if (!first) {
      double kd0[Q0], kd1[Q1];
      kf_ktiles_any<NB0, NB1, true, true>(t, kd0, kd1, lk, L, F.Z0, F.Z1, xrow, valid, g);
      {
#pragma unroll
        for (int q = 0; q < Q0; ++q) kdl[q * 64] = kd0[q];
#pragma unroll
        for (int q = 0; q < Q1; ++q) kdl[(KF_Q + q) * 64] = kd1[q];
      }
    }
    first = false;
    kf_forward_products<NB0, NB1, true>(t, L, F, slot);
    const double gmn = L.gm[pn], gvn = L.gv[pn], dq0n = L.dq0[pn], dq1n = L.dq1[pn];   // zero for padding points (scale 0 in the point-wise kernel)
    double B1[Q1], C1[Q1], sq[Q0];
#pragma unroll
    for (int q = 0; q < Q1; ++q) { B1[q] = 0.0; C1[q] = 0.0; }
#pragma unroll
    for (int q = 0; q < Q0; ++q) sq[q] = t.A0[q] * t.A0[q];
    kf_frag_mm<NB1, Q0>(B1, F.AlT, NB1, Q0, t.K0, slot);
    kf_frag_mm<NB1, Q0>(C1, F.S2T, NB1, Q0, sq, slot);
    double dA0[Q0], dA1[Q1], PdA0[Q0], PdA1[Q1];
#pragma unroll
    for (int q = 0; q < Q0; ++q) { dA0[q] = 2.0 * gvn * t.A0[q] * t.C0[q]; PdA0[q] = 0.0; }
#pragma unroll
    for (int q = 0; q < Q1; ++q) { dA1[q] = 2.0 * gvn * t.A1[q] * C1[q]; PdA1[q] = 0.0; }
    kf_frag_mm<NB0, Q0>(PdA0, F.P0, NB0, Q0, dA0, slot);
    kf_frag_mm<NB1, Q1>(PdA1, F.P1, NB1, Q1, dA1, slot);
    // ---- LDS images for the sums over points (k index = point): K tiles, E tiles
    kf_store_tile<Q0>(bK0, t.K0, g, n);
    kf_store_tile<Q1>(bK1, t.K1, g, n);
    {
      double E0[Q0], E1[Q1];
#pragma unroll
      for (int q = 0; q < Q0; ++q) E0[q] = fma(dq0n, t.K0[q], dA0[q]);
      kf_store_tile<Q0>(c0, E0, g, n);
#pragma unroll
      for (int q = 0; q < Q1; ++q) E1[q] = fma(dq1n, t.K1[q], dA1[q]);
      kf_store_tile<Q1>(c1, E1, g, n);
    }
    kf_wave_sync();
    double gmk[4], gvk[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { gmk[ks] = __shfl(gmn, 4 * ks + g, 64); gvk[ks] = __shfl(gvn, 4 * ks + g, 64); }
    kf_accum<NB0, NB1, 0, true>(accAl, bK0, bK1, gmk, lane);
    kf_accum<NB0, NB0, 0, false>(accP0, c0, bK0, one4, lane);
    kf_accum<NB1, NB1, 0, false>(accP1, c1, bK1, one4, lane);
    kf_wave_sync();
    // B operand of the moment products: lane (kk = g, column j = n) needs psi_j of point 4 ks + g -- loaded here (most of the tile state
    // is dead by now), the round trip hides behind the dS2 products
    double psi[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        // selects, not branches: the eight loads go out back to back (one round trip, not eight)
        const int64_t pt = (int64_t)tile * 16 + 4 * ks + g;
        const double xv = a.X[(pt < a.N ? pt : 0) * a.ldx + psi_col[p]] - psi_zc[p];
        const double v = psi_kind[p] == 0 ? 1.0 : (psi_kind[p] == 1 ? xv : (psi_kind[p] == 2 ? xv * xv : 0.0));
        psi[p][ks] = (pt < a.N) ? v : 0.0;
      }
    kf_store_tile<Q0>(c0, t.A0, g, n);
    kf_store_tile<Q1>(c1, t.A1, g, n);
    kf_wave_sync();
    kf_accum<NB0, NB1, 1, true>(accS2, c0, c1, gvk, lane);
    kf_wave_sync();
    {
      double t0[Q0], t1v[Q1];
#pragma unroll
      for (int q = 0; q < Q0; ++q) t0[q] = fma(gmn, t.B0[q], fma(2.0 * dq0n, t.A0[q], PdA0[q])) * t.K0[q];
      kf_store_tile<Q0>(c0, t0, g, n);
#pragma unroll
      for (int q = 0; q < Q1; ++q) t1v[q] = fma(gmn, B1[q], fma(2.0 * dq1n, t.A1[q], PdA1[q])) * t.K1[q];
      kf_store_tile<Q1>(c1, t1v, g, n);
    }
    kf_wave_sync();
    // moments: acc(rows of factor p, col j) += sum_n t_p[row, n] psi_j(x_n),  psi = {1, xc_d, xc_d^2}
    // (the columns of this chain -- all of an RBF factor, column 0 of a Matern one)
    const bool first0 = (lk & 3) == KERN_RBF || n == 0, first1 = (lk >> 2) == KERN_RBF || n == 0;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int rb = 0; rb < NB0; ++rb) kf_mfma16(accK0[rb], c0[(16 * rb + n) * KF_LD + 4 * ks + g], first0 ? psi[0][ks] : 0.0);
#pragma unroll
      for (int rb = 0; rb < NB1; ++rb) kf_mfma16(accK1[rb], c1[(16 * rb + n) * KF_LD + 4 * ks + g], first1 ? psi[1][ks] : 0.0);
    }
    kf_wave_sync();
    if (lk != 0) {      // the second chain: t' = dK . K' against the remaining columns (wave-uniform: the latent has a Matern factor)
      {
        double t0[Q0], t1v[Q1];
#pragma unroll
        for (int q = 0; q < Q0; ++q) t0[q] = fma(gmn, t.B0[q], fma(2.0 * dq0n, t.A0[q], PdA0[q])) * kdl[q * 64];
        kf_store_tile<Q0>(c0, t0, g, n);
#pragma unroll
        for (int q = 0; q < Q1; ++q) t1v[q] = fma(gmn, B1[q], fma(2.0 * dq1n, t.A1[q], PdA1[q])) * kdl[(KF_Q + q) * 64];
        kf_store_tile<Q1>(c1, t1v, g, n);
      }
      kf_wave_sync();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
        for (int rb = 0; rb < NB0; ++rb) kf_mfma16(accK0[rb], c0[(16 * rb + n) * KF_LD + 4 * ks + g], first0 ? 0.0 : psi[0][ks]);
#pragma unroll
        for (int rb = 0; rb < NB1; ++rb) kf_mfma16(accK1[rb], c1[(16 * rb + n) * KF_LD + 4 * ks + g], first1 ? 0.0 : psi[1][ks]);
      }
      kf_wave_sync();
    }
  }
  // per-wave partials, [block][r][lane]; blocks numbered for the CAPACITY grid (KF_NBMAX x KF_NBMAX) that k_kf_reduce / k_kf_finish index
  double* out = L.acc + (int64_t)w * KF_ACC_DOUBLES;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int rb = 0; rb < NB0; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB1; ++cb) {
        out[((KF_B_AL + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accAl[rb * NB1 + cb][r];
        out[((KF_B_S2 + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accS2[rb * NB1 + cb][r];
      }
#pragma unroll
    for (int rb = 0; rb < NB0; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB0; ++cb) out[((KF_B_P0 + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accP0[rb * NB0 + cb][r];
#pragma unroll
    for (int rb = 0; rb < NB1; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB1; ++cb) out[((KF_B_P1 + rb * KF_NBMAX + cb) * 4 + r) * 64 + lane] = accP1[rb * NB1 + cb][r];
#pragma unroll
    for (int rb = 0; rb < NB0; ++rb) out[((KF_B_K0 + rb) * 4 + r) * 64 + lane] = accK0[rb][r];
#pragma unroll
    for (int rb = 0; rb < NB1; ++rb) out[((KF_B_K1 + rb) * 4 + r) * 64 + lane] = accK1[rb][r];
  }
}
template <int NB0, int NB1>
__global__ void __launch_bounds__(64 * KF_WAVES, 1)
k_kf_backward_kinds(KfArgs a, int kinds) {
  extern __shared__ double lds[];
  kf_backward_kinds_body<NB0, NB1>(a, kinds, lds);
}

// ---- fixed-order sum of the partial accumulators; un-permutes the accumulator layout into row-major matrices ------------------
// block numbering shared by the accumulators of every variant (capacities nb0c, nb1c): Al | S2 (nb0c x nb1c each) | P0 | P1 | K0 | K1
struct KfBlock { int kind, rb, cb; };   // kind 0 Al, 1 S2, 2 P0, 3 P1, 4 moments of factor 0, 5 of factor 1
__device__ __forceinline__ KfBlock kf_block_decode(int blk, int nb0c, int nb1c) {
  KfBlock b;
  const int n01 = nb0c * nb1c;
  if (blk < n01) { b.kind = 0; b.rb = blk / nb1c; b.cb = blk % nb1c; return b; }
  blk -= n01;
  if (blk < n01) { b.kind = 1; b.rb = blk / nb1c; b.cb = blk % nb1c; return b; }
  blk -= n01;
  if (blk < nb0c * nb0c) { b.kind = 2; b.rb = blk / nb0c; b.cb = blk % nb0c; return b; }
  blk -= nb0c * nb0c;
  if (blk < nb1c * nb1c) { b.kind = 3; b.rb = blk / nb1c; b.cb = blk % nb1c; return b; }
  blk -= nb1c * nb1c;
  if (blk < nb0c) { b.kind = 4; b.rb = blk; b.cb = 0; return b; }
  b.kind = 5; b.rb = blk - nb0c; b.cb = 0;
  return b;
}
__host__ __device__ inline int kf_nblocks(int nb0c, int nb1c) { return 2 * nb0c * nb1c + nb0c * nb0c + nb1c * nb1c + nb0c + nb1c; }

// work layout per latent (doubles), R_p = 16 nb_p capacity rows, ldw = max(R0, R1):
//   dAl [R0][ldw] | dS2 [R0][ldw] | dP0 [R0][ldw] | dP1 [R1][ldw] | Kr0 [R0][16] | Kr1 [R1][16]
struct KfWork { int ldw, S2, P0, P1, K0, K1, total; };
__host__ __device__ inline KfWork kf_work_layout(int nb0c, int nb1c) {
  KfWork w;
  const int R0 = 16 * nb0c, R1 = 16 * nb1c;
  w.ldw = R0 > R1 ? R0 : R1;
  w.S2 = R0 * w.ldw; w.P0 = 2 * R0 * w.ldw; w.P1 = 3 * R0 * w.ldw; w.K0 = w.P1 + R1 * w.ldw; w.K1 = w.K0 + R0 * 16; w.total = w.K1 + R1 * 16;
  return w;
}
constexpr int KF_MQ = 16 * KF_NBMAX;
constexpr int KF_W_AL = 0, KF_W_S2 = KF_MQ * KF_MQ, KF_W_P0 = 2 * KF_MQ * KF_MQ, KF_W_P1 = 3 * KF_MQ * KF_MQ, KF_W_K0 = 4 * KF_MQ * KF_MQ,
              KF_W_K1 = KF_W_K0 + KF_MQ * 16, KF_W_TOTAL = KF_W_K1 + KF_MQ * 16;   // = kf_work_layout(KF_NBMAX, KF_NBMAX)
// sums of the point-wise block partials, one workgroup of 256 threads (see k_kron_pw_reduce)
__device__ __forceinline__ void kf_pw_reduce(const double* __restrict__ acc, int blocks, double kl_counted, double* __restrict__ pws) {
  __shared__ double sh[4];
  if (threadIdx.x == 0) pws[7] = kl_counted;   // 1 on the rank(s) that count the KL: summed over ranks like everything else
#pragma unroll
  for (int q = 0; q < KPW_ACC; ++q) {
    double v = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) v += acc[(int64_t)KPW_ACC * b + q];
    v = block_sum<4>(v, sh);
    if (threadIdx.x == 0) pws[q] = v;
  }
}
constexpr int KF_RED_GROUPS = 16;
__global__ void __launch_bounds__(256)
k_kf_reduce(const double* __restrict__ acc0, const double* __restrict__ acc1, int nparts, double* __restrict__ work0, double* __restrict__ work1,
            int nb0c, int nb1c, int nb0_f, int nb1_f, int nb0_g, int nb1_g, const double* __restrict__ pwacc, int pw_blocks, double kl_counted,
            double* __restrict__ pws) {
  if (blockIdx.x == gridDim.x - 1) {          // the extra workgroup(s): the point-wise sums (first latent's only)
    if (blockIdx.y == 0 && pwacc) kf_pw_reduce(pwacc, pw_blocks, kl_counted, pws);
    return;
  }
  __shared__ double sh[KF_RED_GROUPS][16];
  const double* acc = blockIdx.y == 0 ? acc0 : acc1;
  double* work = blockIdx.y == 0 ? work0 : work1;
  const int nb0 = blockIdx.y == 0 ? nb0_f : nb0_g, nb1 = blockIdx.y == 0 ? nb1_f : nb1_g;   // this latent's own block counts (<= capacity)
  const int64_t accd = (int64_t)kf_nblocks(nb0c, nb1c) * 256;
  const int e = blockIdx.x * 16 + (threadIdx.x & 15), grp = threadIdx.x >> 4;
  const int per = (nparts + KF_RED_GROUPS - 1) / KF_RED_GROUPS;
  const int w0 = grp * per, w1 = min(w0 + per, nparts);
  // the point kernels write the accumulator blocks of the latent's OWN grid only: capacity blocks beyond it are never written (and
  // the buffer is never cleared), so they are not read either -- their sums are defined as zero
  bool live;
  {
    const KfBlock b0 = kf_block_decode(e >> 8, nb0c, nb1c);
    const int nr = (b0.kind == 0 || b0.kind == 1 || b0.kind == 2 || b0.kind == 4) ? nb0 : nb1;
    const int nc = (b0.kind == 0 || b0.kind == 1 || b0.kind == 3) ? nb1 : (b0.kind == 2 ? nb0 : 1);
    live = b0.rb < nr && b0.cb < nc;
  }
  double s = 0.0;
  if (live)
    for (int w = w0; w < w1; ++w) s += acc[(int64_t)w * accd + e];
  sh[grp][threadIdx.x & 15] = s;
  __syncthreads();
  if (grp != 0) return;
  double tot = 0.0;
#pragma unroll
  for (int q = 0; q < KF_RED_GROUPS; ++q) tot += sh[q][threadIdx.x & 15];
  // e = (block * 4 + r) * 64 + lane  ->  element (16 rb + 4 r + lane / 16, 16 cb + lane % 16) of its matrix
  const int lane = e & 63, r = (e >> 6) & 3, blk = e >> 8;
  const int ri = 4 * r + (lane >> 4), cj = lane & 15;
  const KfBlock b = kf_block_decode(blk, nb0c, nb1c);
  const KfWork w = kf_work_layout(nb0c, nb1c);
  const int base = b.kind == 0 ? 0 : b.kind == 1 ? w.S2 : b.kind == 2 ? w.P0 : b.kind == 3 ? w.P1 : b.kind == 4 ? w.K0 : w.K1;
  const int ld = b.kind <= 3 ? w.ldw : 16;
  work[base + (16 * b.rb + ri) * ld + 16 * b.cb + cj] = tot;
}

// =============================================================================================================================
// M x M stages
// =============================================================================================================================
struct KfFactorJob {
  const double* Z; int M, D, Mq; const double* hyp;   // Mq = 16 nb; hyp: the factor's record of the device hyperparameter block
  double* zc_out;   // = hyp + KH_ZC, written here: centre of the moment sums (mid-range of Z_p), read by the kernels BEHIND this one
  double* K;        // [128][128] identity padded Kuu factor + jitter (kept for the Kuu-gradient reductions)
  double* P;        // [Mq][Mq] row-major K^-1 (zero padded)
  double* PF;       // fragment order
  double* dvec;     // [Mq] diag(P), then dvec[Mq] = logdet K = sum log L_ii^2
  double* Zs;       // [Mq][D] Z / ell, zero rows beyond M (the point kernels' K tiles)
};
// info: Cholesky status word(s).  own_slots = 0: one word shared by every factor, zeroed by the host (predict).  own_slots = 1: word
// info + 2 * job (an 8-byte slot each, inside the result block that is downloaded anyway); the job's workgroup zeroes its own slot, so
// a step needs neither a memset launch nor a separate status copy.
struct KfFactorArgs { KfFactorJob job[4]; double jitter; double piv_rtol; int* info; int own_slots; };

// fragment image of a row-major matrix: F[(rb * ksn + ks) * 64 + lane] = A(16 rb + lane % 16, 4 ks + lane / 16)   (the A operand of v_mfma_f64_16x16x4)
__device__ __forceinline__ void kf_write_frag(double* __restrict__ F, int nbr, int ksn, int t, int nthreads, const double* __restrict__ A, int64_t lda,
                                              bool transposed) {
  const int total = nbr * ksn * 64;
  for (int idx = t; idx < total; idx += nthreads) {
    const int ln = idx & 63, blk = idx >> 6, ks = blk % ksn, rb = blk / ksn;
    const int row = 16 * rb + (ln & 15), k = 4 * ks + (ln >> 4);
    F[idx] = transposed ? A[(int64_t)k * lda + row] : A[(int64_t)row * lda + k];
  }
}


// One workgroup (1024 threads) per factor: K_p = k_p(Z_p) + jitter I (scripts/onoff.py:188-190), L = chol(K_p) and W = L^-1 in LDS
// (tf.cholesky onofftf/main.py:355; the explicit inverse of scripts/onoff.py:192 is formed as P = W^T W), logdet, diag(P).
__global__ void __launch_bounds__(1024)
k_kf_factor(KfFactorArgs a) {
  extern __shared__ double S[];   // [128][129]
  __shared__ PotrfShared psh;
  __shared__ double red[16];
  const KfFactorJob& jb = a.job[blockIdx.x];
  const int t = threadIdx.x, M = jb.M, Mq = jb.Mq, D = jb.D;
  const auto inv_ell = KF_CONST(jb.hyp) + KH_INV;
  const double var = KF_CONST(jb.hyp)[KH_VAR];
  int* const info = a.own_slots ? a.info + 2 * blockIdx.x : a.info;
  if (a.own_slots && t == 0) { info[0] = 0; info[1] = 0; }       // ordered before the factorisation's atomicCAS by the barriers below
  // inducing inputs into LDS first (the T tiles are idle until the factorisation): with Z read from global memory inside the loop
  // every entry of K sat behind two dependent L2 round trips (in-kernel stamps: 23 k cycles for 16 entries per thread).  K is built
  // for j <= i only and mirrored: rows i and nreal - 1 - i fold into one row of nreal + 1 entries.
  double* zl = &psh.T[0][0][0];
  for (int idx = t; idx < Mq * D; idx += 1024) {
    const int m = idx / D, d = idx - m * D;
    const double z = m < M ? jb.Z[idx] : 0.0;
    zl[idx] = z;
    jb.Zs[idx] = z * inv_ell[d];
  }
  __syncthreads();
  if (t < 64) {        // zc_d = mid-range of the inducing inputs (min / max are exact: any order gives the same bits).  One wave, lanes over the
                       // points: as a serial loop in MAXD lanes (100 dependent LDS reads) this held wave 0 back for ~10 k cycles before its share of K
    for (int d = 0; d < MAXD; ++d) {
      double zc = 0.0;
      if (d < D) {
        double lo = zl[d], hi = lo;                        // point 0: every lane starts from a real value
        for (int m = t; m < M; m += 64) { const double z = zl[m * D + d]; lo = fmin(lo, z); hi = fmax(hi, z); }
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) { lo = fmin(lo, __shfl_xor(lo, sft, 64)); hi = fmax(hi, __shfl_xor(hi, sft, 64)); }
        zc = 0.5 * (lo + hi);
      }
      if (t == 0) jb.zc_out[d] = zc;
    }
  }
  const int nreal = ((M + PNB - 1) / PNB) * PNB;   // the factorisation touches the 32-column panels that hold real rows only
  for (int idx = t; idx < (nreal / 2) * (nreal + 1); idx += 1024) {
    int i = idx / (nreal + 1), j = idx - i * (nreal + 1);
    if (j > i) { j -= i + 1; i = nreal - 1 - i; }
    double v;
    if (i < M && j < M) {
      double r2 = 0.0;
      for (int d = 0; d < D; ++d) { const double q = (zl[i * D + d] - zl[j * D + d]) * inv_ell[d]; r2 = fma(q, q, r2); }
      v = var * exp(-0.5 * r2) + ((i == j) ? a.jitter : 0.0);     // same expression as k_rbf_matrix
    } else {
      v = (i == j) ? 1.0 : 0.0;
    }
    jb.K[i * PB + j] = v;
    S[i * PBLD + j] = v;
    if (i != j) { jb.K[j * PB + i] = v; S[j * PBLD + i] = 0.0; }
  }
  __syncthreads();
  if (!potrf_diag_lds(S, psh, 0, info, (M + PNB - 1) / PNB, true, a.piv_rtol * 2.220446049250313e-16 * (var + a.jitter))) return;   // info = plain 1-based pivot, as on the panel path; the slot says which factor
  // logdet K = sum log L_ii^2 (fixed order: strided partials, then 16 wave sums in order)
  {
    double ld = 0.0;
    for (int i = t; i < M; i += 1024) { const double l = S[i * PBLD + i]; ld += log(l * l); }
    ld = wave_sum(ld);
    if ((t & 63) == 0) red[t >> 6] = ld;
    __syncthreads();
    if (t == 0) { double q = 0.0; for (int w = 0; w < 16; ++w) q += red[w]; jb.dvec[Mq] = q; }
  }
  // P = W^T W on the MFMA pipe, operands straight from the LDS image: W[k][i] (k > i) is S[i][k], the diagonal is dinv, zero above.
  // A(i, k) = W[k][i], B(k, j) = W[k][j].  P is symmetric: blocks rb >= cb only, which need k >= 16 rb; the first four k-steps of a
  // block cross the diagonal of the A rows (and of the B rows when rb == cb) and take the select-guarded reads, the rest read S
  // directly; four k-steps of loads go out together (in-kernel stamps at M = 100: 57 k cycles with one guarded k-step at a time,
  // every LDS round trip exposed).  Dearest blocks first over the 16 waves.  Each lane ends with P(16 rb + 4 r + g, 16 cb + n),
  // r = 0..3 -- one 32-byte granule of the fragment image PF -- and mirrors it into block (cb, rb).
  {
    // (r4: one 16 x 16 x 4 MFMA per k-step; the A operand of a lane is row 16 rb + n of the block -- the same read pattern as the B operand)
    const int lane = t & 63, g = lane >> 4, n = lane & 15, wave = t >> 6;
    const int nbq = Mq / 16, ksn = Mq / 4;
    for (int blk = wave; blk < nbq * (nbq + 1) / 2; blk += 16) {
      int rb = 0, cb = blk;
      while (cb > rb) { cb -= rb + 1; ++rb; }
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const int j = 16 * cb + n, i_a = 16 * rb + n;
      const double* Sb = S + j * PBLD + g;
      const double* Sa = S + i_a * PBLD + g;
      {
        double bv[4], av[4];
        const double dj = psh.dinv[j], di = psh.dinv[i_a];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = 16 * rb + 4 * u + g;
          const double sb = Sb[4 * (4 * rb + u)], sa = Sa[4 * (4 * rb + u)];
          bv[u] = k > j ? sb : (k == j ? dj : 0.0);
          av[u] = k > i_a ? sa : (k == i_a ? di : 0.0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) kf_mfma16(acc, av[u], bv[u]);
      }
      for (int ks = 4 * rb + 4; ks < ksn; ks += 4) {
        double bv[4], av[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { bv[u] = Sb[4 * (ks + u)]; av[u] = Sa[4 * (ks + u)]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) kf_mfma16(acc, av[u], bv[u]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * rb + 4 * r + g;
        const double v = (i < M && j < M) ? acc[r] : 0.0;
        jb.P[i * Mq + j] = v;
        // fragment image (kf_write_frag): element (row R, column C) -> block (R / 16, C / 4), lane R % 16 + 16 (C % 4)
        jb.PF[(int64_t)(rb * ksn + 4 * cb + (n >> 2)) * 64 + 4 * r + g + 16 * (n & 3)] = v;           // (row i, column j)
        if (rb != cb) {
          jb.P[j * Mq + i] = v;
          jb.PF[(int64_t)(cb * ksn + 4 * rb + r) * 64 + n + 16 * g] = v;                              // (row j, column i): the mirror
        }
        if (i == j) jb.dvec[i] = v;
      }
    }
  }
}
// k_kf_factor_kinds: a Matern factor's K_p as k_kron_matern_matrix builds it -- matern_k off the diagonal, the formula at r2 = 0
// (r = 1e-6) plus jitter on it, identity in the padding; kinds: bit 2 j = the kind of job j.
__device__ __forceinline__ void kf_factor_kinds_body(const KfFactorArgs& a, int kinds, double* S, PotrfShared& psh, double* red) {
  const KfFactorJob& jb = a.job[blockIdx.x];
  const int kind = (kinds >> (2 * blockIdx.x)) & 3;
  const int t = threadIdx.x, M = jb.M, Mq = jb.Mq, D = jb.D;
  const auto inv_ell = KF_CONST(jb.hyp) + KH_INV;
  const double var = KF_CONST(jb.hyp)[KH_VAR];
  int* const info = a.own_slots ? a.info + 2 * blockIdx.x : a.info;
  if (a.own_slots && t == 0) { info[0] = 0; info[1] = 0; }       // ordered before the factorisation's atomicCAS by the barriers below
  // inducing inputs into LDS first (the T tiles are idle until the factorisation): with Z read from global memory inside the loop
  // every entry of K sat behind two dependent L2 round trips (in-kernel stamps: 23 k cycles for 16 entries per thread).  K is built
  // for j <= i only and mirrored: rows i and nreal - 1 - i fold into one row of nreal + 1 entries.
  double* zl = &psh.T[0][0][0];
  for (int idx = t; idx < Mq * D; idx += 1024) {
    const int m = idx / D, d = idx - m * D;
    const double z = m < M ? jb.Z[idx] : 0.0;
    zl[idx] = z;
    jb.Zs[idx] = z * inv_ell[d];
  }
  __syncthreads();
  if (t < 64) {        // zc_d = mid-range of the inducing inputs (min / max are exact: any order gives the same bits).  One wave, lanes over the
                       // points: as a serial loop in MAXD lanes (100 dependent LDS reads) this held wave 0 back for ~10 k cycles before its share of K
    for (int d = 0; d < MAXD; ++d) {
      double zc = 0.0;
      if (d < D) {
        double lo = zl[d], hi = lo;                        // point 0: every lane starts from a real value
        for (int m = t; m < M; m += 64) { const double z = zl[m * D + d]; lo = fmin(lo, z); hi = fmax(hi, z); }
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) { lo = fmin(lo, __shfl_xor(lo, sft, 64)); hi = fmax(hi, __shfl_xor(hi, sft, 64)); }
        zc = 0.5 * (lo + hi);
      }
      if (t == 0) jb.zc_out[d] = zc;
    }
  }
  const int nreal = ((M + PNB - 1) / PNB) * PNB;   // the factorisation touches the 32-column panels that hold real rows only
  for (int idx = t; idx < (nreal / 2) * (nreal + 1); idx += 1024) {
    int i = idx / (nreal + 1), j = idx - i * (nreal + 1);
    if (j > i) { j -= i + 1; i = nreal - 1 - i; }
    double v;
    if (i < M && j < M) {
      double r2 = 0.0;
      for (int d = 0; d < D; ++d) { const double q = (zl[i * D + d] - zl[j * D + d]) * inv_ell[d]; r2 = fma(q, q, r2); }
      if (kind != KERN_RBF) v = matern_k(kind, var, r2) + ((i == j) ? a.jitter : 0.0);
      else v = var * exp(-0.5 * r2) + ((i == j) ? a.jitter : 0.0);     // same expression as k_rbf_matrix
    } else {
      v = (i == j) ? 1.0 : 0.0;
    }
    jb.K[i * PB + j] = v;
    S[i * PBLD + j] = v;
    if (i != j) { jb.K[j * PB + i] = v; S[j * PBLD + i] = 0.0; }
  }
  __syncthreads();
  if (!potrf_diag_lds(S, psh, 0, info, (M + PNB - 1) / PNB, true, a.piv_rtol * 2.220446049250313e-16 * (var + a.jitter))) return;   // info = plain 1-based pivot, as on the panel path; the slot says which factor
  // logdet K = sum log L_ii^2 (fixed order: strided partials, then 16 wave sums in order)
  {
    double ld = 0.0;
    for (int i = t; i < M; i += 1024) { const double l = S[i * PBLD + i]; ld += log(l * l); }
    ld = wave_sum(ld);
    if ((t & 63) == 0) red[t >> 6] = ld;
    __syncthreads();
    if (t == 0) { double q = 0.0; for (int w = 0; w < 16; ++w) q += red[w]; jb.dvec[Mq] = q; }
  }
  // P = W^T W on the MFMA pipe, operands straight from the LDS image: W[k][i] (k > i) is S[i][k], the diagonal is dinv, zero above.
  // A(i, k) = W[k][i], B(k, j) = W[k][j].  P is symmetric: blocks rb >= cb only, which need k >= 16 rb; the first four k-steps of a
  // block cross the diagonal of the A rows (and of the B rows when rb == cb) and take the select-guarded reads, the rest read S
  // directly; four k-steps of loads go out together (in-kernel stamps at M = 100: 57 k cycles with one guarded k-step at a time,
  // every LDS round trip exposed).  Dearest blocks first over the 16 waves.  Each lane ends with P(16 rb + 4 r + g, 16 cb + n),
  // r = 0..3 -- one 32-byte granule of the fragment image PF -- and mirrors it into block (cb, rb).
  {
    // (r4: one 16 x 16 x 4 MFMA per k-step; the A operand of a lane is row 16 rb + n of the block -- the same read pattern as the B operand)
    const int lane = t & 63, g = lane >> 4, n = lane & 15, wave = t >> 6;
    const int nbq = Mq / 16, ksn = Mq / 4;
    for (int blk = wave; blk < nbq * (nbq + 1) / 2; blk += 16) {
      int rb = 0, cb = blk;
      while (cb > rb) { cb -= rb + 1; ++rb; }
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const int j = 16 * cb + n, i_a = 16 * rb + n;
      const double* Sb = S + j * PBLD + g;
      const double* Sa = S + i_a * PBLD + g;
      {
        double bv[4], av[4];
        const double dj = psh.dinv[j], di = psh.dinv[i_a];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = 16 * rb + 4 * u + g;
          const double sb = Sb[4 * (4 * rb + u)], sa = Sa[4 * (4 * rb + u)];
          bv[u] = k > j ? sb : (k == j ? dj : 0.0);
          av[u] = k > i_a ? sa : (k == i_a ? di : 0.0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) kf_mfma16(acc, av[u], bv[u]);
      }
      for (int ks = 4 * rb + 4; ks < ksn; ks += 4) {
        double bv[4], av[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { bv[u] = Sb[4 * (ks + u)]; av[u] = Sa[4 * (ks + u)]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) kf_mfma16(acc, av[u], bv[u]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * rb + 4 * r + g;
        const double v = (i < M && j < M) ? acc[r] : 0.0;
        jb.P[i * Mq + j] = v;
        // fragment image (kf_write_frag): element (row R, column C) -> block (R / 16, C / 4), lane R % 16 + 16 (C % 4)
        jb.PF[(int64_t)(rb * ksn + 4 * cb + (n >> 2)) * 64 + 4 * r + g + 16 * (n & 3)] = v;           // (row i, column j)
        if (rb != cb) {
          jb.P[j * Mq + i] = v;
          jb.PF[(int64_t)(cb * ksn + 4 * rb + r) * 64 + n + 16 * g] = v;                              // (row j, column i): the mirror
        }
        if (i == j) jb.dvec[i] = v;
      }
    }
  }
}
__global__ void __launch_bounds__(1024)
k_kf_factor_kinds(KfFactorArgs a, int kinds) {
  extern __shared__ double S[];   // [128][129]
  __shared__ PotrfShared psh;
  __shared__ double red[16];
  kf_factor_kinds_body(a, kinds, S, psh, red);
}

// ---- small dense algebra of the M x M stages: every operand lives in LDS with row stride KF_SLD (odd: column walks are conflict free)
constexpr int KF_SLD = KF_MQ + 1;
constexpr int KF_SMAT = KF_MQ * KF_SLD;
// C (m x n) = op(A) (m x k) * op(B) (k x n) [+ C]; m, n, k multiples of 16; the caller synchronises.  One wave per 16 x 16 block of C
// on the MFMA pipe (operands straight from the row-major LDS images; 8 k-steps of four 4x4x4 products at 32 points).  The first
// version gave every thread one element of C and a scalar loop over k: 64 LDS reads per thread and product, 2-3 us for each of the
// five chained products of k_kf_finish.
template <bool TA, bool TB, bool ACC>
__device__ __forceinline__ void kf_lds_mm(double* C, const double* A, const double* B, int m, int n, int k, int w0 = 0) {
  // w0: first wave of this product (independent products of one phase start on different waves: a 32 x 32 product is four blocks)
  const int nwaves = blockDim.x >> 6, wave = ((threadIdx.x >> 6) + nwaves - w0) % nwaves, lane = threadIdx.x & 63;
  const int kq = lane >> 4, bj = lane & 15, ci = lane >> 4;
  const int nbn = n / 16, nblk = (m / 16) * nbn;
  for (int blk = wave; blk < nblk; blk += nwaves) {
    const int rb = blk / nbn, cb = blk - rb * nbn;
    double acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = ACC ? C[(16 * rb + 4 * r + ci) * KF_SLD + 16 * cb + bj] : 0.0;
    for (int ks = 0; ks < k / 4; ++ks) {      // one 16 x 16 x 4 product per k-step: A (row l % 16, k l / 16), B (k l / 16, column l % 16)
      const int q = 4 * ks + kq;
      const double b = TB ? B[(16 * cb + bj) * KF_SLD + q] : B[q * KF_SLD + 16 * cb + bj];
      const int i = 16 * rb + bj;
      const double a = TA ? A[q * KF_SLD + i] : A[i * KF_SLD + q];
      kf_mfma16(acc, a, b);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(16 * rb + 4 * r + ci) * KF_SLD + 16 * cb + bj] = acc[r];
  }
}
// The same product with one thread per element of C and k summed in ascending order (the first version of these kernels).  Kept
// for the first phase of k_kf_finish (dP_p += dAlpha T^T, Q_p, X, dU): everything there is multiplied by P_p = K_p^-1 on both sides
// afterwards, and at cond(K_s) ~ 5e7 (the pptr initialisation) the summation order of these inputs moves the last digits of
// d var / d ell around the op-order floor of tests/test_gpu_pptr_params.py -- the MFMA order put d var_g at 3.3x the floor (and d ell_g
// at 0.5x instead of 1x), this order keeps the 2.3x the test has always seen.  Neither is more accurate against the 40-digit values.
template <bool TA, bool TB, bool ACC>
__device__ __forceinline__ void kf_lds_mm_seq(double* C, const double* A, const double* B, int m, int n, int k) {
  for (int idx = threadIdx.x; idx < m * n; idx += blockDim.x) {
    const int i = idx / n, j = idx - i * n;
    double v = 0.0;
#pragma unroll 4
    for (int q = 0; q < k; ++q) v = fma(TA ? A[q * KF_SLD + i] : A[i * KF_SLD + q], TB ? B[j * KF_SLD + q] : B[q * KF_SLD + j], v);
    if (ACC) C[i * KF_SLD + j] += v; else C[i * KF_SLD + j] = v;
  }
}
// ---- compensated (two-double) products for the P_p sandwich of the reverse pass -------------------------------------------------
// dK_p = -P_p sym(dP_p) P_p is where the factored reverse pass loses its digits on an ill-conditioned factor: the entries of P_p = K_p^-1
// are ~cond(K_p) / var in size with alternating signs and the products cancel down to the gradient.  CPU experiment with a working
// precision per stage (tools/dd_experiment.py; pptr init, 32 x 32 grid, cond(K_s) = 5e7, largest d ELBO / d Z_s entry): everything in
// float64 1.7e-3; THESE TWO PRODUCTS carried in twice the precision (inputs and result plain float64) 1.1e-8; nothing else matters
// (the inverse itself, Alpha, the sums over points, the reductions against K_p: unchanged results in 106 bits).  Error-free
// transformations: Knuth's two-sum, the FMA two-product; the running sum is (hi, lo), lo collects every rounding error (Ogita, Rump &
// Oishi's Dot2: the result is as accurate as if computed in doubled precision and rounded once).  Contraction must stay off inside.
__device__ __forceinline__ void kf_dd_mac(double& sh, double& sl, double a, double b) {          // (sh, sl) += a b
#pragma clang fp contract(off)
  const double p = a * b;
  const double e = __builtin_fma(a, b, -p);
  const double s = sh + p;
  const double bb = s - sh;
  const double err = (sh - (s - bb)) + (p - bb);
  sh = s;
  sl += err + e;
}
__device__ __forceinline__ void kf_dd_mac2(double& sh, double& sl, double a, double bh, double bl) {   // (sh, sl) += a (bh + bl)
#pragma clang fp contract(off)
  const double p = a * bh;
  const double e = __builtin_fma(a, bl, __builtin_fma(a, bh, -p));
  const double s = sh + p;
  const double bb = s - sh;
  const double err = (sh - (s - bb)) + (p - bb);
  sh = s;
  sl += err + e;
}
// (Ch, Cl) = A B, one thread per element, A / B float64 LDS images (row stride KF_SLD); result normalised (|Cl| <= ulp(Ch) / 2)
__device__ __forceinline__ void kf_lds_mm_dd(double* Ch, double* Cl, const double* A, const double* B, int m, int n, int k) {
  for (int idx = threadIdx.x; idx < m * n; idx += blockDim.x) {
    const int i = idx / n, j = idx - i * n;
    double sh = 0.0, sl = 0.0;
#pragma unroll 4
    for (int q = 0; q < k; ++q) kf_dd_mac(sh, sl, A[i * KF_SLD + q], B[q * KF_SLD + j]);
    const double h = sh + sl;
    Ch[i * KF_SLD + j] = h;
    Cl[i * KF_SLD + j] = sl - (h - sh);
  }
}
// G = -(A (Bh + Bl)) - coef A2, rounded once to float64 (A2 = the matrix whose multiple is subtracted: P_p, KL logdet term)
__device__ __forceinline__ void kf_lds_mm_dd2_neg(double* G, const double* A, const double* Bh, const double* Bl, const double* A2, double coef, int m, int n,
                                                  int k) {
  for (int idx = threadIdx.x; idx < m * n; idx += blockDim.x) {
    const int i = idx / n, j = idx - i * n;
    double sh = 0.0, sl = 0.0;
#pragma unroll 4
    for (int q = 0; q < k; ++q) kf_dd_mac2(sh, sl, A[i * KF_SLD + q], Bh[q * KF_SLD + j], Bl[q * KF_SLD + j]);
    kf_dd_mac(sh, sl, coef, A2[i * KF_SLD + j]);
    G[i * KF_SLD + j] = -(sh + sl);
  }
}
__device__ __forceinline__ void kf_lds_load(double* dst, const double* __restrict__ src, int rows, int cols, int ld) {
  for (int idx = threadIdx.x; idx < rows * cols; idx += blockDim.x) { const int i = idx / cols, j = idx - i * cols; dst[i * KF_SLD + j] = src[(int64_t)i * ld + j]; }
}
__device__ __forceinline__ void kf_lds_store(double* __restrict__ dst, const double* src, int rows, int cols, int ld) {
  for (int idx = threadIdx.x; idx < rows * cols; idx += blockDim.x) { const int i = idx / cols, j = idx - i * cols; dst[(int64_t)i * ld + j] = src[i * KF_SLD + j]; }
}
// fragment image of an LDS matrix (see kf_write_frag)
__device__ __forceinline__ void kf_lds_frag(double* __restrict__ F, int nbr, int ksn, const double* A, bool transposed) {
  const int total = nbr * ksn * 64;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int ln = idx & 63, blk = idx >> 6, ks = blk % ksn, rb = blk / ksn;
    const int row = 16 * rb + (ln & 15), k = 4 * ks + (ln >> 4);
    F[idx] = transposed ? A[k * KF_SLD + row] : A[row * KF_SLD + k];
  }
}

struct KfLatentJob {
  int M0, M1, Mq0, Mq1;
  const double *P0, *P1, *dvec0, *dvec1;     // from k_kf_factor
  const double *PF0, *PF1;                   // their fragment images (larger-grid kernels)
  const double *u, *s;                       // [M0*M1] from the parameter pack
  double *U, *S2, *T0, *T1, *Al;             // [Mq0][Mq1] zero padded: U, s^2, U P1, P0 U, Alpha = P0 U P1
  double *AlF, *S2F, *AlTF, *S2TF;           // fragment images
  double* klv;                               // [8]: sum U.Alpha, sum log s^2, sum d0 d1 s^2, logdet K0, logdet K1
};
struct KfLatentArgs { KfLatentJob job[2]; };

__global__ void __launch_bounds__(1024)
k_kf_latent(KfLatentArgs a) {
  __shared__ double sm[7 * KF_SMAT];
  __shared__ double sh[3][16];
  double *sP0 = sm, *sP1 = sm + KF_SMAT, *sU = sm + 2 * KF_SMAT, *sS2 = sm + 3 * KF_SMAT, *sT = sm + 4 * KF_SMAT, *sAl = sm + 5 * KF_SMAT,
         *sT1 = sm + 6 * KF_SMAT;
  const KfLatentJob& jb = a.job[blockIdx.x];
  const int t = threadIdx.x, M0 = jb.M0, M1 = jb.M1, Mq0 = jb.Mq0, Mq1 = jb.Mq1;
  kf_lds_load(sP0, jb.P0, Mq0, Mq0, Mq0);
  kf_lds_load(sP1, jb.P1, Mq1, Mq1, Mq1);
  for (int idx = t; idx < Mq0 * Mq1; idx += 1024) {
    const int i = idx / Mq1, j = idx - i * Mq1;
    const bool in = i < M0 && j < M1;
    const double sv = in ? jb.s[i * M1 + j] : 0.0, uv = in ? jb.u[i * M1 + j] : 0.0;
    sU[i * KF_SLD + j] = uv; sS2[i * KF_SLD + j] = sv * sv;
    jb.U[idx] = uv; jb.S2[idx] = sv * sv;
  }
  __syncthreads();
  kf_lds_mm<false, false, false>(sT1, sP0, sU, Mq0, Mq1, Mq0);      // T1 = P0 U
  kf_lds_mm<false, false, false>(sT, sU, sP1, Mq0, Mq1, Mq1, 4);    // T0 = U P1   (independent: same phase, own buffer, other waves)
  __syncthreads();
  kf_lds_store(jb.T1, sT1, Mq0, Mq1, Mq1);
  kf_lds_store(jb.T0, sT, Mq0, Mq1, Mq1);
  kf_lds_mm<false, false, false>(sAl, sP0, sT, Mq0, Mq1, Mq0);      // Alpha = P0 (U P1)   (= __kron_mv, scripts/onoff.py:193)
  __syncthreads();
  kf_lds_store(jb.Al, sAl, Mq0, Mq1, Mq1);
  kf_lds_frag(jb.AlF, Mq0 / 16, Mq1 / 4, sAl, false);
  kf_lds_frag(jb.S2F, Mq0 / 16, Mq1 / 4, sS2, false);
  kf_lds_frag(jb.AlTF, Mq1 / 16, Mq0 / 4, sAl, true);
  kf_lds_frag(jb.S2TF, Mq1 / 16, Mq0 / 4, sS2, true);
  // KL scalars (GaussKLkron, onofftf/main.py:350-387, factored): fixed-order sums
  double av = 0.0, bv = 0.0, cv = 0.0;
  for (int idx = t; idx < M0 * M1; idx += 1024) {
    const int i = idx / M1, j = idx - i * M1;
    const double sv = jb.s[idx];
    av = fma(sU[i * KF_SLD + j], sAl[i * KF_SLD + j], av);
    bv += log(sv * sv);
    cv = fma(jb.dvec0[i] * jb.dvec1[j], sv * sv, cv);
  }
  double vals[3] = {av, bv, cv};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double v = wave_sum(vals[q]);
    if ((t & 63) == 0) sh[q][t >> 6] = v;
  }
  __syncthreads();
  if (t < 3) { double r = 0.0; for (int w = 0; w < 16; ++w) r += sh[t][w]; jb.klv[t] = r; }
  if (t == 0) { jb.klv[3] = jb.dvec0[Mq0]; jb.klv[4] = jb.dvec1[Mq1]; }
}

// One workgroup per latent: the M x M reverse pass.  Inputs: the summed accumulators (k_kf_reduce) and the forward matrices.
//   dU = P0 dAl P1 ;  dP0 += dAl T0^T ;  dP1 += T1^T dAl                                   (Alpha = P0 U P1)
//   KL:  dP_p -= 1/4 (Q_p + Q_p^T) + 1/2 diag(w_p),  Q0 = T0 U^T, Q1 = U^T T1, w0_i = sum_j d1_j s2_ij, w1_j = sum_i d0_i s2_ij
//   dK_p = -P_p sym(dP_p) P_p - kl * 1/2 M_other P_p  ->  Kuu-style reductions against K_p into krow_p; data moments added
//   gu = dU - kl Alpha ;  gs = 2 s dS2 - kl (-1/s + d0_i d1_j s)
struct KfFinishJob {
  int M0, M1, Mq0, Mq1, D0, D1;
  const double *P0, *P1, *dvec0, *dvec1, *K0, *K1, *Z0, *Z1;
  const double *PF0, *PF1;
  const double *hyp0, *hyp1;          // the two factors' records of the device hyperparameter block (zc: centre of the moment sums)
  const double *U, *S2, *T0, *T1, *Al, *s;
  const double* work;  // KF_W_TOTAL summed accumulators
  double *krow0, *krow1, *gu, *gs;     // outputs: [M0][2 + 2 D0], [M1][2 + 2 D1], [M0*M1], [M0*M1]
};
struct KfFinishArgs { KfFinishJob job[2]; double jitter; int with_kl; };
constexpr size_t KF_FIN_LDS = sizeof(double) * 10 * KF_SMAT;

// grid (2, latents): workgroup (p, h) runs the reverse pass of factor p of latent h; workgroup p = 0 also forms dU -> gu, gs
__global__ void __launch_bounds__(1024)
k_kf_finish(KfFinishArgs a) {
  extern __shared__ double sm[];
  double *sP = sm, *sPo = sm + KF_SMAT, *sdAl = sm + 2 * KF_SMAT, *sdP = sm + 3 * KF_SMAT, *sT = sm + 4 * KF_SMAT, *sU = sm + 5 * KF_SMAT,
         *sX = sm + 6 * KF_SMAT, *sG = sm + 7 * KF_SMAT, *sQ = sm + 8 * KF_SMAT, *sK = sm + 9 * KF_SMAT;
  const KfFinishJob& jb = a.job[blockIdx.y];
  const int p = blockIdx.x;
  const int t = threadIdx.x, M0 = jb.M0, M1 = jb.M1, Mq0 = jb.Mq0, Mq1 = jb.Mq1;
  const bool kl = a.with_kl != 0;
  const int M = p == 0 ? M0 : M1, Mq = p == 0 ? Mq0 : Mq1, Mo = p == 0 ? M1 : M0, D = p == 0 ? jb.D0 : jb.D1;
  const double* Z = p == 0 ? jb.Z0 : jb.Z1;
  const auto zc = KF_CONST(p == 0 ? jb.hyp0 : jb.hyp1) + KH_ZC;
  const double* Kr = jb.work + (p == 0 ? KF_W_K0 : KF_W_K1);
  double* krow = p == 0 ? jb.krow0 : jb.krow1;
  kf_lds_load(sP, p == 0 ? jb.P0 : jb.P1, Mq, Mq, Mq);
  kf_lds_load(sdAl, jb.work + KF_W_AL, Mq0, Mq1, KF_MQ);
  kf_lds_load(sdP, jb.work + (p == 0 ? KF_W_P0 : KF_W_P1), Mq, Mq, KF_MQ);
  kf_lds_load(sT, p == 0 ? jb.T0 : jb.T1, Mq0, Mq1, Mq1);
  kf_lds_load(sU, jb.U, Mq0, Mq1, Mq1);
  kf_lds_load(sK, p == 0 ? jb.K0 : jb.K1, M, M, PB);
  if (p == 0) kf_lds_load(sPo, jb.P1, Mq1, Mq1, Mq1);
  // small per-row operands of the later phases in LDS: the inducing inputs and (KL) w_i = sum_o d_o S2[i, o] -- read inside serial loops
  // they cost an L2 round trip per element (the diagonal threads of the X phase walked 32 of them one after the other)
  __shared__ double sZ[KF_MQ * MAXD], sW[KF_MQ];
  for (int idx = t; idx < M * D; idx += 1024) sZ[idx] = Z[idx];
  if (kl) {
    const int i = t >> 5, l = t & 31;        // 32 lanes per row
    double w = 0.0;
    if (i < M) {
      if (p == 0) { for (int o = l; o < M1; o += 32) w = fma(jb.dvec1[o], jb.S2[i * Mq1 + o], w); }
      else { for (int o = l; o < M0; o += 32) w = fma(jb.dvec0[o], jb.S2[o * Mq1 + i], w); }
    }
#pragma unroll
    for (int sft = 16; sft >= 1; sft >>= 1) w += __shfl_xor(w, sft, 64);
    if (l == 0 && i < KF_MQ) sW[i] = w;
  }
  __syncthreads();
  if (p == 0) {
    // (rounds 3: these ran one thread per element with k in ascending order, to keep the last digits of d var / d ell where a test's
    // "op-order floor" margin had seen them; with the compensated sandwich below that margin is gone -- section 1 of HISTORY.md -- and
    // the products are back on the MFMA pipe, the independent ones of the phase on different waves)
    kf_lds_mm<false, false, false>(sX, sdAl, sPo, Mq0, Mq1, Mq1);           // X = dAl P1
    kf_lds_mm<false, true, true>(sdP, sdAl, sT, Mq0, Mq0, Mq1, 4);          // dP0 += dAl T0^T
    if (kl) kf_lds_mm<false, true, false>(sQ, sT, sU, Mq0, Mq0, Mq1, 8);    // Q0 = T0 U^T
    __syncthreads();
    kf_lds_mm<false, false, false>(sG, sP, sX, Mq0, Mq1, Mq0);              // dU = P0 X
    __syncthreads();
    for (int idx = t; idx < M0 * M1; idx += 1024) {
      const int i = idx / M1, j = idx - i * M1;
      const double sv = jb.s[idx];
      double gu = sG[i * KF_SLD + j], gs = 2.0 * sv * jb.work[KF_W_S2 + i * KF_MQ + j];
      if (kl) { gu -= jb.Al[i * Mq1 + j]; gs -= (-1.0 / sv + jb.dvec0[i] * jb.dvec1[j] * sv); }
      jb.gu[idx] = gu; jb.gs[idx] = gs;
    }
  } else {
    kf_lds_mm<true, false, true>(sdP, sT, sdAl, Mq1, Mq1, Mq0);             // dP1 += T1^T dAl
    if (kl) kf_lds_mm<true, false, false>(sQ, sU, sT, Mq1, Mq1, Mq0, 4);    // Q1 = U^T T1
  }
  __syncthreads();
  // sX = sym(dP) [- kl pieces]
  for (int idx = t; idx < Mq * Mq; idx += 1024) {
    const int i = idx / Mq, j = idx - i * Mq;
    double v = 0.5 * (sdP[i * KF_SLD + j] + sdP[j * KF_SLD + i]);
    if (kl) {
      v -= 0.25 * (sQ[i * KF_SLD + j] + sQ[j * KF_SLD + i]);
      if (i == j) v -= 0.5 * sW[i];
    }
    sX[i * KF_SLD + j] = v;
  }
  __syncthreads();
  // G = -P sym(dP) P - coef P in compensated arithmetic (kf_dd_mac, above): Q = sym(dP) P as (hi, lo) -- lo in the dead dP buffer --
  // then P (Q_hi + Q_lo) + coef P summed in (hi, lo) and rounded once
  kf_lds_mm_dd(sQ, sdP, sX, sP, Mq, Mq, Mq);
  __syncthreads();
  const double coef = kl ? 0.5 * (double)Mo : 0.0;
  kf_lds_mm_dd2_neg(sG, sP, sQ, sdP, sP, coef, Mq, Mq, Mq);
  __syncthreads();
  // krow[m][c]: Kuu part (as k_kuu_grad, Kz = K_p - jitter I) + data moments rebuilt around z_m
  // eight lanes per (m, c) entry sweep j (fixed-order tree over the eight partial sums)
  const int W = 2 + 2 * D;
  for (int base = 0; base < M * W; base += 128) {
    const int idx = base + (t >> 3), l = t & 7;
    const bool on = idx < M * W;
    const int m = on ? idx / W : 0, c = on ? idx - m * W : 0;
    double v = 0.0;
    const int d = (c == 0) ? 0 : (c - 1) % D;
    const double zm = sZ[m * D + d];
    if (on && c <= 2 * D) {
      for (int j = l; j < M; j += 8) {
        const double kz = sK[m * KF_SLD + j] - ((m == j) ? a.jitter : 0.0);
        const double tt = sG[m * KF_SLD + j] * kz;
        const double df = sZ[j * D + d] - zm;
        v += (c == 0) ? tt : ((c <= D) ? 2.0 * tt * df : tt * df * df);
      }
    }
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    if (on && l == 0) {
      if (c <= 2 * D) {
        const double s0 = Kr[m * 16];
        if (c == 0) v += s0;
        else {
          const double dz = zm - zc[d], s1 = Kr[m * 16 + 1 + d];
          if (c <= D) v += s1 - dz * s0;
          else v += Kr[m * 16 + 1 + D + d] - 2.0 * dz * s1 + dz * dz * s0;
        }
      }
      krow[idx] = v;
    }
  }
}
// ---- Matern factors, small grids: the krow rows of a Matern factor WITHOUT a Matern form of k_kf_finish ----
// (A second instantiation of the finish body beside k_kf_finish changed the register allocation the compiler gives k_kf_finish itself,
// and that kernel's machine code is pinned.)  What a Matern factor needs from the finish stage differs from the RBF form in two places
// only: the moment columns 1 .. 2 D of krow take G . K'_p where RBF takes G . (K_p - jitter I), and their data moments are re-centred with
// sum t' (column 15 of the moment block) where RBF uses sum t (column 0).  Both are INPUTS of k_kf_finish -- the K_p image it reads and the
// moment block of its work buffer -- so the step runs k_kf_finish twice: once as always (gu, gs, column 0 of krow, and every column of an
// RBF factor), and once on a copy of its inputs in which K_p is K'_p(Z_p, Z_p) and column 0 of the moment block holds column 15
// (k_kf_kd_prepare), writing to scratch outputs; k_kf_krow_merge then takes the columns 1 .. 2 D of the Matern factors from the second run.
// On the diagonal of K' the differences z_j - z_m are zero, so its value there (and the jitter k_kf_finish subtracts from it) adds nothing.
// Per latent in KfState::spill (unused by the small grids otherwise):  Kd0 [32][PB] | Kd1 [32][PB] | work' | krow0' | krow1' | gu' | gs'
constexpr int KF_KD_K = KF_MQ * PB, KF_KD_WORK = 2 * KF_KD_K, KF_KD_KROW0 = KF_KD_WORK + KF_W_TOTAL, KF_KD_KROW1 = KF_KD_KROW0 + KF_MQ * (2 + 2 * MAXD),
              KF_KD_GU = KF_KD_KROW1 + KF_MQ * (2 + 2 * MAXD), KF_KD_GS = KF_KD_GU + KF_MQ * KF_MQ, KF_KD_TOTAL = KF_KD_GS + KF_MQ * KF_MQ;
struct KfKdJob { int M0, M1, D0, D1; const double *Z0, *Z1, *hyp0, *hyp1; const double* work; double* buf; double *krow0, *krow1; };
struct KfKdArgs { KfKdJob job[2]; };
// grid (3, latents): workgroups 0 / 1 build K'_p of a Matern factor p, workgroup 2 copies the work block with sum t' in column 0 of the
// moment block of every Matern factor
__global__ void __launch_bounds__(256)
k_kf_kd_prepare(KfKdArgs a, int kinds) {
  const KfKdJob& jb = a.job[blockIdx.y];
  const int t = threadIdx.x;
  if (blockIdx.x == 2) {
    double* w = jb.buf + KF_KD_WORK;
    for (int idx = t; idx < KF_W_TOTAL; idx += 256) {
      double v = jb.work[idx];
      if (idx >= KF_W_K0) {
        const int p = idx >= KF_W_K1 ? 1 : 0, e = idx - (p ? KF_W_K1 : KF_W_K0);
        if ((e & 15) == 0 && kf_kind_of(kinds, blockIdx.y, p) != KERN_RBF) v = jb.work[idx + 15];
      }
      w[idx] = v;
    }
    return;
  }
  const int p = blockIdx.x, kind = kf_kind_of(kinds, blockIdx.y, p);
  if (kind == KERN_RBF) return;      // its columns come from the first run
  const int M = p == 0 ? jb.M0 : jb.M1, D = p == 0 ? jb.D0 : jb.D1;
  const double* Z = p == 0 ? jb.Z0 : jb.Z1;
  const auto hyp = KF_CONST(p == 0 ? jb.hyp0 : jb.hyp1);
  const auto inv_ell = hyp + KH_INV;
  const double var = hyp[KH_VAR];
  double* Kd = jb.buf + p * KF_KD_K;
  for (int idx = t; idx < M * M; idx += 256) {
    const int i = idx / M, j = idx - i * M;
    double r2 = 0.0;
    for (int d = 0; d < D; ++d) { const double q = (Z[i * D + d] - Z[j * D + d]) * inv_ell[d]; r2 = fma(q, q, r2); }
    Kd[i * PB + j] = matern_kd(kind, var, r2);
  }
}
// grid (2, latents): columns 1 .. 2 D of the krow rows of a Matern factor from the second run
__global__ void __launch_bounds__(256)
k_kf_krow_merge(KfKdArgs a, int kinds) {
  const KfKdJob& jb = a.job[blockIdx.y];
  const int p = blockIdx.x;
  if (kf_kind_of(kinds, blockIdx.y, p) == KERN_RBF) return;
  const int M = p == 0 ? jb.M0 : jb.M1, D = p == 0 ? jb.D0 : jb.D1, W = 2 + 2 * D;
  const double* src = jb.buf + (p == 0 ? KF_KD_KROW0 : KF_KD_KROW1);
  double* dst = p == 0 ? jb.krow0 : jb.krow1;
  for (int idx = threadIdx.x; idx < M * W; idx += 256) {
    const int c = idx % W;
    if (c >= 1 && c <= 2 * D) dst[idx] = src[idx];
  }
}

}  // namespace zigp

namespace zigp {

#include "zigp_kronl.h"

// =============================================================================================================================
// host orchestration
// =============================================================================================================================
constexpr size_t KF_BWD_LDS = sizeof(double) * (KF_WAVES * 4 * 16 * KF_NBMAX * KF_LD + 6 * KF_FRAG + 2 * KF_MQ_ * MAXD);
struct KfState {
  DevBuf in, mat, pts, acc, res, out, spill, fit;
};

// Variants of the point-stage kernels by capacity (16-row blocks per factor):
//   small  <2, 2>  accumulators in registers (grids up to 32 x 32: BASELINE cfg5)
//   large  <1, 7>  operands spilled per tile, k_kfl_accum (the reference's [10, 100] grid, scripts/onoff.py:52-53)
// anything else (and more than 7 input columns per factor: 1 + 2 D moment columns <= 16) takes the GEMM-panel path of zigp_kron.hip.
// tests/test_gpu_kron_nd.py walks this table (every factor dimension 1 to 8, each instantiation, latents with different block counts).
struct KfPlan { bool ok, large; int nb0c, nb1c; };
static KfPlan kf_plan(const zigp_kron_params* p, int nlat) {
  KfPlan pl = {false, false, 0, 0};
  if (p->D0 > 7 || p->D1 > 7) return pl;
  const int m0 = std::max(p->M0f, nlat == 2 ? p->M0g : 0), m1 = std::max(p->M1f, nlat == 2 ? p->M1g : 0);
  if (m0 <= 16 * KF_NBMAX && m1 <= 16 * KF_NBMAX) { pl.ok = true; pl.nb0c = KF_NBMAX; pl.nb1c = KF_NBMAX; return pl; }
  if (m0 <= 16 && m1 <= 112) { pl.ok = true; pl.large = true; pl.nb0c = 1; pl.nb1c = 7; return pl; }
  return pl;
}
static bool kf_eligible(const zigp_kron_params* p, int nlat) { return kf_plan(p, nlat).ok; }

// launch helpers: the small-grid kernels are instantiated for the exact block counts (1 or 2 per factor)
template <int NB0, int NB1>
static int kf_launch_small(zigp_ctx* c, bool backward, dim3 grid, const KfArgs& ka) {
  if (backward) {
    static bool attr = false;
    if (!attr) {
      ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kf_backward<NB0, NB1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KF_BWD_LDS));
      attr = true;
    }
    hipLaunchKernelGGL((k_kf_backward<NB0, NB1>), grid, dim3(64 * KF_WAVES), KF_BWD_LDS, c->stream, ka);
  } else {
    hipLaunchKernelGGL((k_kf_forward<NB0, NB1>), grid, dim3(64 * KF_WAVES), 0, c->stream, ka);
  }
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
// the _kinds instantiations (a call with a Matern factor): the packed kinds ride as an argument of their own; the backward kernel keeps
// a lane-private K' image per wave behind the fragment images
static_assert(sizeof(KfFac) == 40 && sizeof(KfLat) == 168 && sizeof(KfArgs) == 384, "the arguments of the RBF point kernels do not move");
constexpr size_t KF_BWD_LDS_KINDS = KF_BWD_LDS + sizeof(double) * KF_WAVES * 2 * KF_Q * 64;
static_assert(KF_BWD_LDS_KINDS <= 160 * 1024, "k_kf_backward_kinds: LDS of one workgroup");
template <int NB0, int NB1>
static int kf_launch_small_kinds(zigp_ctx* c, bool backward, dim3 grid, const KfArgs& ka, int kinds) {
  if (backward) {
    static bool attr = false;
    if (!attr) {
      ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kf_backward_kinds<NB0, NB1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KF_BWD_LDS_KINDS));
      attr = true;
    }
    hipLaunchKernelGGL((k_kf_backward_kinds<NB0, NB1>), grid, dim3(64 * KF_WAVES), KF_BWD_LDS_KINDS, c->stream, ka, kinds);
  } else {
    hipLaunchKernelGGL((k_kf_forward_kinds<NB0, NB1>), grid, dim3(64 * KF_WAVES), 0, c->stream, ka, kinds);
  }
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}
static int kf_launch_small(zigp_ctx* c, int nb0, int nb1, bool backward, dim3 grid, const KfArgs& ka, int kinds) {
  if (kinds) {
    if (nb0 == 1 && nb1 == 1) return kf_launch_small_kinds<1, 1>(c, backward, grid, ka, kinds);
    if (nb0 == 1 && nb1 == 2) return kf_launch_small_kinds<1, 2>(c, backward, grid, ka, kinds);
    if (nb0 == 2 && nb1 == 1) return kf_launch_small_kinds<2, 1>(c, backward, grid, ka, kinds);
    return kf_launch_small_kinds<2, 2>(c, backward, grid, ka, kinds);
  }
  if (nb0 == 1 && nb1 == 1) return kf_launch_small<1, 1>(c, backward, grid, ka);
  if (nb0 == 1 && nb1 == 2) return kf_launch_small<1, 2>(c, backward, grid, ka);
  if (nb0 == 2 && nb1 == 1) return kf_launch_small<2, 1>(c, backward, grid, ka);
  return kf_launch_small<2, 2>(c, backward, grid, ka);
}
// one launch for both latents when their block counts agree, else one per latent (KfArgs::lat0 selects it)
static int kf_launch_small_latents(zigp_ctx* c, const int (*Mq)[2], int nlat, bool backward, unsigned gx, KfArgs& ka, int kinds) {
  const bool same = nlat == 1 || (Mq[0][0] == Mq[1][0] && Mq[0][1] == Mq[1][1]);
  if (same) { ka.lat0 = 0; return kf_launch_small(c, Mq[0][0] / 16, Mq[0][1] / 16, backward, dim3(gx, nlat), ka, kinds); }
  for (int h = 0; h < nlat; ++h) { ka.lat0 = h; ZIGP_TRY(kf_launch_small(c, Mq[h][0] / 16, Mq[h][1] / 16, backward, dim3(gx, 1), ka, kinds)); }
  ka.lat0 = 0;
  return 0;
}

constexpr int KF_KROW_W = 2 + 2 * MAXD;

// Fixed-order sums of the point-wise block partials -> pws[0..KPW_ACC) (kf_pw_reduce, above): the result block of a step has a size
// that depends on the inducing grid only (never on the shard), so a data-parallel run can sum it over ranks in place (comm_allreduce).
// Value-only steps launch it on its own; gradient steps run it as one extra workgroup of k_kf_reduce (a launch less on a step that is
// launch-bound at minibatch size).
__global__ void __launch_bounds__(256)
k_kron_pw_reduce(const double* __restrict__ acc, int blocks, double kl_counted, double* __restrict__ pws) { kf_pw_reduce(acc, blocks, kl_counted, pws); }

// =============================================================================================================================
// device-resident fit loop (zigp_kron_fit_steps): free state -> parameter image, result block -> Adam update
// =============================================================================================================================
// The reference's fit is 50 000 minibatch steps of one model shape (scripts/onoff.py:375-381), each: gradient of cost = -(scale data - KL)
// (:318,334), chained through the Log1pe transforms of the positive parameters (:88-123), one tf.train.AdamOptimizer per learning
// rate (:325-350; TF defaults beta1 .9, beta2 .999, eps 1e-8, lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)).  Here the parameter image
// the kernels read is produced ON THE DEVICE from the free state (k_fit_update), so n steps are enqueued back to back on one stream and
// the host synchronises once per call.  Block order of the flat free-state vector (ZIGP_FIT_BLOCKS = 17): for latent f, then g:
// Z0, Z1, u, s, ell0, ell1, var0, var1; then the likelihood variance.
// The single-latent heads (zigp_kron_head_fit_steps; svgp.py:240-330, classifier.py:276-316, the regression loop of hurdle.py) run the same
// steps with nlat = 1 and the HEAD instantiation of the update kernel: ZIGP_HEAD_FIT_BLOCKS = 10 blocks -- the eight of latent f, the
// likelihood variance (-> KH_NOISE, gradient pws[1]) and f_mu (-> KH_FMU, gradient pws[4]) -- of which any may be untrainable.
constexpr int KFIT_BLOCKS = ZIGP_FIT_BLOCKS;
static_assert(ZIGP_HEAD_FIT_BLOCKS <= KFIT_BLOCKS, "the head layout uses the first blocks of the descriptor");
struct KfFitDesc {
  int off[KFIT_BLOCKS], n[KFIT_BLOCKS], dst[KFIT_BLOCKS], positive[KFIT_BLOCKS];   // offset in the free vector, size, offset in the parameter image
  int trainable[KFIT_BLOCKS];   // HEAD only: 0 = the block keeps its x, m, v (its value is still the transform of its free entry)
  double lr[KFIT_BLOCKS];
  int nlat, D0, D1, M[2][2], Mq[2][2];
  int off_z[2][2], off_hyp, off_hyp2;          // parameter image; the two hyperparameter blocks (step i reads block i % 2, its update writes the other)
  int big_blk[8], big_off[9], hyp_blk[9], hyp_off[10];   // thread -> element map of k_fit_update: the big blocks (Z, u, s) in order, then the hyperparameter blocks in a workgroup of their own
                                                         // (a layout with fewer blocks repeats the total in the offsets it does not use)
  int res_size, res_krow0, res_krow1, res_gu, res_gs, res_pws, res_info;   // result block (doubles)
  double beta1, beta2, eps;
};
struct KfFitArgs {
  KfFitDesc d;
  double *x, *m, *v;            // free state and Adam moments [n_free]
  double* img;                  // parameter image (KfState::in)
  const double* res;            // result block of the step that just ran
  double* hist;                 // [n_steps][2]: data term, KL
  int* fail;                    // [4]: 0 = fine, else {1 + step, factor job, pivot}
  int step;                     // index within this call
  double lr_sq, lr_den;         // sqrt(1 - beta2^t), 1 - beta1^t of this step (computed on the host exactly as zigp.optim.AdamGroups does)
  int update;                   // 0: only free state -> image (first launch of a call)
};

// kfit_softplus (Log1pe forward) and kfit_adam (the Adam arithmetic) are shared with the dense fit loop: zigp_kernels.h
__device__ __forceinline__ double kfit_value(const KfFitDesc& d, int b, double x) { return d.positive[b] ? kfit_softplus(x) : x; }

// Thread -> element of the free vector.  Workgroups 0 .. G - 2 walk the big blocks (Z0, Z1, u, s of f, then of g) one element per thread;
// the LAST workgroup owns every hyperparameter element (ell, var of both latents, the noise: <= 33), which need the sums over the
// inducing rows.  Returns the block (or -1) and the index inside it.
__device__ __forceinline__ int kfit_element(const KfFitDesc& d, int& i) {
  const bool hyper_wg = blockIdx.x == gridDim.x - 1;
  const int j = hyper_wg ? (int)threadIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int nb = hyper_wg ? 9 : 8;
  const int* off = hyper_wg ? d.hyp_off : d.big_off;
  const int* blk = hyper_wg ? d.hyp_blk : d.big_blk;
  if (j >= off[nb]) { i = 0; return -1; }
  int k = 0;
  for (int q = 1; q < nb; ++q) k += (j >= off[q]) ? 1 : 0;
  i = j - off[k];
  return blk[k];
}

// kind of block b: 0 Z0, 1 Z1, 2 u, 3 s, 4 ell0, 5 ell1, 6 var0, 7 var1, 8 noise, 9 f_mu (HEAD only: there the block index is the kind)
template <bool HEAD>
__device__ __forceinline__ int kfit_kind(int b, int& h) {
  if (HEAD) { h = 0; return b; }
  h = b / 8;
  return b == KFIT_BLOCKS - 1 ? 8 : b % 8;
}

// value of element (block b, index i) into the parameter image: plain blocks are copied, the hyperparameter blocks fill their records of
// the hyper block Hn the NEXT step reads (the block the current step was evaluated at stays intact: two blocks, used in turn)
template <bool HEAD>
__device__ __forceinline__ void kfit_store_value(const KfFitArgs& a, double* Hn, int b, int i, double val) {
#pragma clang fp contract(off)
  const KfFitDesc& d = a.d;
  int h;
  const int kind = kfit_kind<HEAD>(b, h);
  if (kind <= 3) a.img[d.dst[b] + i] = val;
  else if (kind <= 5) { double* R = Hn + (2 * h + (kind - 4)) * KH_FAC; R[KH_ELL + i] = val; R[KH_INV + i] = 1.0 / val; }
  else if (kind <= 7) Hn[(2 * h + (kind - 6)) * KH_FAC + KH_VAR] = val;
  else if (kind == 8) Hn[KH_NOISE] = val;
  else Hn[KH_FMU] = val;
}

// Grid: KFIT_THREADS-wide workgroups, one element of the free vector per thread (the update is ~300 fp64 instructions per element --
// tanh, log1p, exp, sqrt, divisions: in ONE workgroup it took 20 us of a 105 us step, VALU-bound on a single compute unit).  The blocks
// are laid out so that the few hyperparameter elements (ell, var, noise: those that need the sums over the inducing rows) come LAST
// in the element order handled by the last workgroup, which also writes the history entry and the failure record.
constexpr int KFIT_MROWS = 16 * 7;       // most inducing rows per factor on the fused path (kf_plan)
constexpr int KFIT_THREADS = 256;
// HEAD: the single-latent block layout (see KfFitDesc) -- the noise takes pws[1], f_mu takes pws[4] (the sum of the fmean cotangents), and a
// block with trainable = 0 only re-derives its value (the hyperparameter block it lives in changes every step).  The on/off instantiation
// (!HEAD) is the kernel as it was: same element map, same operations in the same order.
template <bool HEAD>
__global__ void __launch_bounds__(KFIT_THREADS)
k_fit_update(KfFitArgs a) {
  const KfFitDesc& d = a.d;
  const int t = threadIdx.x;
  const double* Ho = a.img + (a.step & 1 ? d.off_hyp2 : d.off_hyp);      // the block this step's kernels read
  double* Hn = a.img + (a.update ? (a.step & 1 ? d.off_hyp : d.off_hyp2) : d.off_hyp);      // the block the next step will read
  int i = 0;
  const int b = kfit_element(d, i);
  const int e = b >= 0 ? d.off[b] + i : 0;
  if (!a.update) {                       // first launch of a call: free state -> parameter image
    if (b >= 0) kfit_store_value<HEAD>(a, Hn, b, i, kfit_value(d, b, a.x[e]));
    return;
  }
  __shared__ int s_fail;
  __shared__ double s_col[2][2][MAXD + 1][KFIT_MROWS];      // the columns of krow that are summed over the inducing rows
  __shared__ double s_dl[2][2][MAXD], s_dv[2][2];
  const bool hyper_wg = blockIdx.x == gridDim.x - 1;         // owns every ell / var / noise element (see the host side: those blocks are its last elements)
  if (t == 0) {
    int f = a.fail[0];
    if (f == 0) {
      const int* info = reinterpret_cast<const int*>(a.res + d.res_info);
      int bad = -1;
      for (int j = 2 * d.nlat - 1; j >= 0; --j) bad = info[2 * j] != 0 ? j : bad;      // independent loads, first failing job wins
      if (bad >= 0) { f = 1 + a.step; if (hyper_wg) { a.fail[1] = bad; a.fail[2] = info[2 * bad]; a.fail[0] = f; } }
    }
    s_fail = f;
  }
  if (hyper_wg) {   // stage the krow columns whose sums over the rows make d ell / d var (all loads in flight together) ...
    for (int idx = t; idx < 4 * (MAXD + 1) * KFIT_MROWS; idx += KFIT_THREADS) {
      const int mm = idx % KFIT_MROWS, c = (idx / KFIT_MROWS) % (MAXD + 1), q = (idx / (KFIT_MROWS * (MAXD + 1))) & 1, h = idx / (2 * KFIT_MROWS * (MAXD + 1));
      const int D = q == 0 ? d.D0 : d.D1, W = 2 + 2 * D;
      if (h < d.nlat && c <= D && mm < d.M[h][q])
        s_col[h][q][c][mm] = a.res[h * d.res_size + (q == 0 ? d.res_krow0 : d.res_krow1) + mm * W + (c == D ? 0 : 1 + D + c)];
    }
  }
  // this thread's element: every load up front
  int kind = 0, h = 0;
  double x = 0.0, mv = 0.0, vv = 0.0, gnum = 0.0, aux = 1.0;
  const double* pws = a.res + d.res_pws;
  if (b >= 0) {
    kind = kfit_kind<HEAD>(b, h);
    const double* R = a.res + h * d.res_size;
    x = a.x[e]; mv = a.m[e]; vv = a.v[e];
    if (kind <= 1) {
      const int q = kind, D = q == 0 ? d.D0 : d.D1, W = 2 + 2 * D, mm = i / D, dd = i - mm * D;
      aux = Ho[(2 * h + q) * KH_FAC + KH_ELL + dd];
      gnum = R[(q == 0 ? d.res_krow0 : d.res_krow1) + mm * W + 1 + dd];
    } else if (kind == 2) gnum = R[d.res_gu + i];
    else if (kind == 3) gnum = R[d.res_gs + i];
    else if (kind <= 5) aux = Ho[(2 * h + (kind - 4)) * KH_FAC + KH_ELL + i];
    else if (kind <= 7) aux = Ho[(2 * h + (kind - 6)) * KH_FAC + KH_VAR];
    else gnum = pws[kind == 8 ? 1 : 4];      // d noise; HEAD: d f_mu = the sum of the fmean cotangents
  }
  __syncthreads();
  if (s_fail) return;             // a Cholesky failed in this or an earlier step of the call: the state stays as it was before that step
  if (hyper_wg) {
    // ... and sum them in the host's order (m = 0, 1, ...), one thread each, from LDS
    if (t < 4 * (MAXD + 1)) {
      const int hh = t / (2 * (MAXD + 1)), q = (t / (MAXD + 1)) & 1, dd = t % (MAXD + 1), D = q == 0 ? d.D0 : d.D1;
      if (hh < d.nlat && dd <= D) {
        double sm = 0.0;
        for (int mm = 0; mm < d.M[hh][q]; ++mm) sm += s_col[hh][q][dd][mm];
        if (dd == D) s_dv[hh][q] = sm; else s_dl[hh][q][dd] = sm;
      }
    }
    if (t == 64) {    // history of the step: data term, KL from its five scalars per latent (as kronf_run assembles it)
#pragma clang fp contract(off)
      double klsum = 0.0;
      const double kl_ranks = pws[7];
      if (kl_ranks > 0.0)
        for (int hh = 0; hh < d.nlat; ++hh) {
          const double* vk = a.res + hh * d.res_size;
          const int M0 = d.M[hh][0], M1 = d.M[hh][1];
          klsum += 0.5 * (vk[0] - kl_ranks * (double)M0 * M1 - vk[1] + vk[2] + (double)M1 * vk[3] + (double)M0 * vk[4]);
        }
      a.hist[2 * a.step] = pws[0];
      a.hist[2 * a.step + 1] = klsum;
    }
    __syncthreads();
  }
  if (b < 0) return;
  {
#pragma clang fp contract(off)
    double gc;      // d ELBO / d (constrained value)
    if (kind <= 1) gc = gnum / (aux * aux);
    else if (kind <= 3 || kind >= 8) gc = gnum;
    else if (kind <= 5) gc = s_dl[h][kind - 4][i] / (aux * aux * aux);
    else gc = s_dv[h][kind - 6] / aux + pws[2 + h] * Ho[(2 * h + 1 - (kind - 6)) * KH_FAC + KH_VAR];   // Knn = var0 var1 enters var_n directly (scripts/onoff.py:196-200)
    // cost = -ELBO, chained through the transform, one Adam step (kfit_adam, zigp_kernels.h)
    double xnew = x, mnew = mv, vnew = vv;
    if (!HEAD || d.trainable[b]) {
      kfit_adam(gc, d.positive[b] != 0, d.lr[b], KfitAdam{d.beta1, d.beta2, d.eps, a.lr_sq, a.lr_den}, xnew, mnew, vnew);
      a.m[e] = mnew; a.v[e] = vnew; a.x[e] = xnew;
    }
    kfit_store_value<HEAD>(a, Hn, b, i, kfit_value(d, b, xnew));
  }
}

struct KfFitCall {          // host side of one zigp_kron_fit_steps / zigp_kron_head_fit_steps call
  const char* name;          // the entry point, for its messages
  bool head;                 // single-latent block layout (ZIGP_HEAD_FIT_BLOCKS)
  const double* lr; const int32_t* positive; const int32_t* trainable;   // per block; trainable: head only (nullptr = every block)
  double beta1, beta2, eps;
  double *x, *m, *v; int64_t n_free;
  int64_t t0; int n_steps; const int64_t* row_begin; int64_t batch;
  const double *Xw, *Yw;     // host batches for steps with row_begin < 0 (batch -(1 + k) of them)
  double *hist_data, *hist_kl;
};

// Host image H [KH_SIZE] of the device hyperparameter block (KH_*, zigp_kernels.h) of a call that stages its parameters: one record per
// (latent, factor) -- 1 / ell, ell, the variance; KH_ZC, the centre of the moment sums, is filled in by k_kf_factor -- and the noise.
// KH_FMU stays 0: outside a fit call f_mu travels by value.
static void kf_fill_hyp(double* H, const KronHostLatent* hl, int nlat, int D0, int D1, double noise) {
  memset(H, 0, sizeof(double) * KH_SIZE);
  for (int h = 0; h < nlat; ++h)
    for (int q = 0; q < 2; ++q) {
      const int D = q == 0 ? D0 : D1;
      double* Rh = H + (2 * h + q) * KH_FAC;
      for (int d = 0; d < MAXD; ++d) {
        Rh[KH_INV + d] = d < D ? 1.0 / hl[h].ell[q][d] : 0.0;
        Rh[KH_ELL + d] = d < D ? hl[h].ell[q][d] : 0.0;
      }
      Rh[KH_VAR] = hl[h].var[q];
    }
  H[KH_NOISE] = noise;
}

// Test hook of a step (zigp_test_kron_fused_step, include/zigp_diag.h).  Each tap is a device-to-device copy enqueued on the step's
// stream right behind the launch that produces the value, into a buffer of its own; flush() downloads them once the step has finished.
struct KfTap {
  const zigp_stage_kron_fused* s;
  struct Snap { double* host; DevBuf dev; size_t n; };
  std::vector<Snap> snaps;
  DevBuf inject[2];       // device copies of the injected cotangents [4][N], uploaded before the step
  int64_t facts[ZIGP_KFF_COUNT];
  int snap(zigp_ctx* c, double* host, const double* dev, size_t n) {
    if (!host || n == 0) return 0;
    snaps.emplace_back();
    Snap& q = snaps.back();
    q.host = host; q.n = n;
    ZIGP_ENSURE(c, q.dev, n);
    ZIGP_HIP(c, hipMemcpyAsync(q.dev.p, dev, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  int flush(zigp_ctx* c) {      // the stream is idle
    for (Snap& q : snaps) ZIGP_HIP(c, hipMemcpy(q.host, q.dev.p, sizeof(double) * q.n, hipMemcpyDeviceToHost));
    if (s->facts) memcpy(s->facts, facts, sizeof(facts));
    return 0;
  }
};

// Per-call state of the fused path: the plan, the layout of its device buffers and everything else the launches of a step need that
// does not change between the steps of a call.  kf_prepare builds it once; the fit loop runs kf_step on it up to hundreds of times (a step
// is launch-bound) and moves d_hyp only.
struct KfRun {
  zigp_ctx* c;
  const KronCall* k;
  const KfFitCall* fit;       // nullptr outside a fit call
  KfState* ks;
  KfPlan pl;
  KfWork wl;
  int nlat, D0, D1, ldx, nblk, pw_blocks;
  int64_t N, Npad;
  bool need_grad;
  int kinds;                  // the factor kinds of the call, packed (kf_kind_of); 0 = every factor RBF: the RBF kernels, else their _kinds forms
  int Mq[2][2];
  bool large_exact;           // every latent has exactly the capacity's block counts: the instantiation with compile-time bounds
  size_t lds_fwd, lds_bwd;    // LDS of the larger-grid point kernels: fragment images packed by the actual block counts (max over the latents)
  // per-factor region of KfState::mat: K [128][128] | P | PF | dvec | Zs ; per-latent: U S2 T0 T1 Al | AlF S2F AlTF S2TF | work | scratch
  size_t FAC_P, FAC_PF, FAC_DV, FAC_ZS, FAC_SIZE;
  size_t LAT_U, LAT_S2, LAT_T0, LAT_T1, LAT_AL, LAT_ALF, LAT_S2F, LAT_ALTF, LAT_S2TF, LAT_WORK, LAT_SCR, SCR_SET, LAT_SIZE;
  // result block: [latent f][latent g][pws: 8 sums over points][4 Cholesky status slots (8 doubles)]; everything in front of the status
  // slots is summed over ranks in a data-parallel run; behind them, not downloaded: the point-wise block partials
  size_t RES_KLV, RES_KROW0, RES_KROW1, RES_GU, RES_GS, RES_SIZE, RES_PWS, RES_INFO, n_res;
  // the staged image (one host -> device copy): the PARAMETER IMAGE -- per latent Z0, Z1, u, s, then the hyperparameter block (KH_*) --
  // followed by X, Y of a host minibatch.  In a fit call the parameter image is written by k_fit_update instead, and a second
  // hyperparameter block follows the first: step i reads block i % 2, its update writes the other.
  size_t off_z[2][2], off_u[2], off_s[2], off_hyp, off_hyp2, off_x, off_y, n_in;
  size_t n_wrap;              // fit: host batches behind the image, [k][N][ldx], then their Y [k][N]
  size_t pts_lat;             // per latent in KfState::pts: part[4], gm, gv, dq0, dq1
  double* d_hyp;              // the hyperparameter block the next step's kernels read
  double *d_wrap, *d_pwacc;
  int* hinfo;                 // predict: the status word on its way to the host
  double* fac(int h, int q) const { return ks->mat.p + (size_t)(2 * h + q) * FAC_SIZE; }
  double* lat(int h) const { return ks->mat.p + (size_t)4 * FAC_SIZE + (size_t)h * LAT_SIZE; }
  double* pts(int h) const { return ks->pts.p + (size_t)h * pts_lat; }
  double* res(int h) const { return ks->res.p + (size_t)h * RES_SIZE; }
};

static int kf_prepare(zigp_ctx* c, const KronCall& k, const KfFitCall* fit, KfRun& s) {
  memset(&s, 0, sizeof(s));
  s.c = c; s.k = &k; s.fit = fit;
  s.nlat = k.nlat; s.need_grad = k.need_grad; s.N = k.N;
  for (int h = 0; h < k.nlat; ++h)
    for (int q = 0; q < 2; ++q) s.kinds |= (k.hl[h].kind[q] & 3) << (2 * (2 * h + q));
  const KfPlan pl = s.pl = kf_plan(k.p, k.nlat);
  if (!c->kronf) { c->kronf.reset(new (std::nothrow) KfState()); if (!c->kronf) { c->err = "out of memory"; return ZIGP_EHIP; } }
  KfState& ks = *c->kronf;
  s.ks = &ks;
  ZIGP_TRY(begin_staged_call(c));
  const KronHostLatent* hl = k.hl;
  const int nlat = s.nlat, D0 = s.D0 = k.p->D0, D1 = s.D1 = k.p->D1, ldx = s.ldx = D0 + D1;
  const int64_t N = s.N;
  s.Npad = std::max<int64_t>(1024, round_up(N, 1024));
  // ---- sizes of this variant
  const int R0 = 16 * pl.nb0c, R1 = 16 * pl.nb1c;
  const KfWork wl = s.wl = kf_work_layout(pl.nb0c, pl.nb1c);
  s.nblk = kf_nblocks(pl.nb0c, pl.nb1c);
  const size_t r01 = (size_t)R0 * R1, rmax = (size_t)wl.ldw * wl.ldw;
  s.FAC_P = (size_t)PB * PB; s.FAC_PF = s.FAC_P + rmax; s.FAC_DV = s.FAC_PF + rmax; s.FAC_ZS = s.FAC_DV + wl.ldw + 8; s.FAC_SIZE = s.FAC_ZS + (size_t)wl.ldw * MAXD;
  s.LAT_U = 0; s.LAT_S2 = r01; s.LAT_T0 = 2 * r01; s.LAT_T1 = 3 * r01; s.LAT_AL = 4 * r01; s.LAT_ALF = 5 * r01; s.LAT_S2F = 6 * r01; s.LAT_ALTF = 7 * r01;
  s.LAT_S2TF = 8 * r01; s.LAT_WORK = 9 * r01; s.LAT_SCR = s.LAT_WORK + wl.total; s.SCR_SET = 3 * rmax + r01 + wl.ldw; s.LAT_SIZE = s.LAT_SCR + 2 * s.SCR_SET;
  s.RES_KLV = 0; s.RES_KROW0 = 8; s.RES_KROW1 = s.RES_KROW0 + (size_t)R0 * KF_KROW_W; s.RES_GU = s.RES_KROW1 + (size_t)R1 * KF_KROW_W;
  s.RES_GS = s.RES_GU + r01; s.RES_SIZE = s.RES_GS + r01;
  s.RES_PWS = (size_t)2 * s.RES_SIZE; s.RES_INFO = s.RES_PWS + 8; s.n_res = s.RES_INFO + 8;
  size_t off = 0;
  for (int h = 0; h < nlat; ++h) {
    s.off_z[h][0] = off; off += (size_t)hl[h].M[0] * D0;
    s.off_z[h][1] = off; off += (size_t)hl[h].M[1] * D1;
    s.off_u[h] = off; off += (size_t)hl[h].M[0] * hl[h].M[1];
    s.off_s[h] = off; off += (size_t)hl[h].M[0] * hl[h].M[1];
  }
  s.off_hyp = off; off += KH_SIZE;
  s.off_hyp2 = off; off += KH_SIZE;
  s.off_x = off; s.off_y = k.dev_xy ? s.off_x : s.off_x + (size_t)N * ldx;
  s.n_in = k.dev_xy ? off : s.off_y + (size_t)N;
  if (fit)
    for (int i = 0; i < fit->n_steps; ++i)
      if (fit->row_begin[i] < 0) s.n_wrap = std::max<size_t>(s.n_wrap, (size_t)(-fit->row_begin[i]));
  s.pw_blocks = (int)(s.Npad / PW_THREADS);
  s.pts_lat = (size_t)8 * s.Npad;
  ZIGP_ENSURE(c, ks.in, s.n_in + s.n_wrap * (size_t)N * (ldx + 1));
  ZIGP_ENSURE(c, ks.mat, (size_t)4 * s.FAC_SIZE + 2 * s.LAT_SIZE);
  ZIGP_ENSURE(c, ks.pts, 2 * s.pts_lat);
  ZIGP_ENSURE(c, ks.res, s.n_res + (size_t)s.pw_blocks * KPW_ACC);
  s.d_hyp = ks.in.p + s.off_hyp;
  s.d_wrap = ks.in.p + s.n_in;
  s.d_pwacc = ks.res.p + s.n_res;
  for (int h = 0; h < nlat; ++h)
    for (int q = 0; q < 2; ++q) s.Mq[h][q] = (int)round_up(hl[h].M[q], 16);
  s.large_exact = pl.large;
  for (int h = 0; h < nlat; ++h) s.large_exact = s.large_exact && s.Mq[h][0] == 16 * pl.nb0c && s.Mq[h][1] == 16 * pl.nb1c;
  for (int h = 0; h < nlat; ++h) {
    const size_t b0 = s.Mq[h][0] / 16, b1 = s.Mq[h][1] / 16;
    s.lds_fwd = std::max(s.lds_fwd, sizeof(double) * 256 * (b0 * b0 + b1 * b1 + 2 * b0 * b1));
    s.lds_bwd = std::max(s.lds_bwd, sizeof(double) * 256 * (b0 * b0 + b1 * b1 + 4 * b0 * b1));
  }
  return 0;
}

// the dynamic-LDS limits of the kernels launched below, once per process (k_kf_backward's: kf_launch_small)
static int kf_set_attributes(zigp_ctx* c) {
  static bool attr_set = false;
  if (attr_set) return 0;
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kf_factor), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * PB * PBLD)));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kf_finish), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KF_FIN_LDS));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_forward<1, 7, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_backward<1, 7, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_forward<1, 7, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_backward<1, 7, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_latent), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kfl_latent_lds(16 * 7)));
  // the _kinds forms (Matern factors)
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kf_factor_kinds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * PB * PBLD)));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_forward_kinds<1, 7, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_backward_kinds<1, 7, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_forward_kinds<1, 7, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kfl_backward_kinds<1, 7, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  attr_set = true;
  return 0;
}

// the parameter image and, for a host minibatch, its rows: one staged copy (a fit call writes its image on the device: kf_fit_run)
static int kf_stage_inputs(KfRun& s) {
  zigp_ctx* c = s.c;
  const KronCall& k = *s.k;
  const KronHostLatent* hl = k.hl;
  ZIGP_PINNED(c, hin, s.n_in);
  if (!k.dev_xy) {
    memcpy(hin + s.off_x, k.X, sizeof(double) * s.N * s.ldx);
    if (k.Y) memcpy(hin + s.off_y, k.Y, sizeof(double) * s.N); else memset(hin + s.off_y, 0, sizeof(double) * s.N);
  }
  for (int h = 0; h < s.nlat; ++h) {
    memcpy(hin + s.off_z[h][0], hl[h].Z[0], sizeof(double) * hl[h].M[0] * s.D0);
    memcpy(hin + s.off_z[h][1], hl[h].Z[1], sizeof(double) * hl[h].M[1] * s.D1);
    memcpy(hin + s.off_u[h], hl[h].u, sizeof(double) * hl[h].M[0] * hl[h].M[1]);
    memcpy(hin + s.off_s[h], hl[h].s, sizeof(double) * hl[h].M[0] * hl[h].M[1]);
  }
  kf_fill_hyp(hin + s.off_hyp, hl, s.nlat, s.D0, s.D1, k.p->noise);
  ZIGP_HIP(c, hipMemcpyAsync(s.ks->in.p, hin, sizeof(double) * s.n_in, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ---- the stages of ONE step on rows (Xd, Yd), in launch order -- everything else a step reads lives on the device (parameter image,
// hyper block).  TAP: the step of the stage tests, with a snapshot behind each launch; an ordinary step is the instantiation without them.
template <bool TAP>
static int kf_stage_factor(KfRun& s, KfTap* tap) {
  zigp_ctx* c = s.c;
  KfFactorArgs fa;
  memset(&fa, 0, sizeof(fa));
  for (int h = 0; h < s.nlat; ++h)
    for (int q = 0; q < 2; ++q) {
      KfFactorJob& jb = fa.job[2 * h + q];
      jb.Z = s.ks->in.p + s.off_z[h][q]; jb.M = s.k->hl[h].M[q]; jb.D = q == 0 ? s.D0 : s.D1; jb.Mq = s.Mq[h][q];
      jb.hyp = s.d_hyp + (2 * h + q) * KH_FAC; jb.zc_out = s.d_hyp + (2 * h + q) * KH_FAC + KH_ZC;
      jb.K = s.fac(h, q); jb.P = s.fac(h, q) + s.FAC_P; jb.PF = s.fac(h, q) + s.FAC_PF; jb.dvec = s.fac(h, q) + s.FAC_DV; jb.Zs = s.fac(h, q) + s.FAC_ZS;
    }
  fa.jitter = s.k->jitter; fa.piv_rtol = c->pivot_rtol;
  if (s.k->predict) { fa.info = c->d_info; fa.own_slots = 0; }
  else { fa.info = reinterpret_cast<int*>(s.ks->res.p + s.RES_INFO); fa.own_slots = 1; }
  if (s.kinds) hipLaunchKernelGGL(k_kf_factor_kinds, dim3(2 * s.nlat), dim3(1024), sizeof(double) * PB * PBLD, c->stream, fa, s.kinds);
  else hipLaunchKernelGGL(k_kf_factor, dim3(2 * s.nlat), dim3(1024), sizeof(double) * PB * PBLD, c->stream, fa);
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) {
    for (int h = 0; h < s.nlat; ++h)
      for (int q = 0; q < 2; ++q) {
        const zigp_kronf_tap_factor& tf = tap->s->lat[h].fac[q];
        const KfFactorJob& jb = fa.job[2 * h + q];
        const size_t mq = (size_t)jb.Mq;
        ZIGP_TRY(tap->snap(c, tf.K, jb.K, (size_t)PB * PB)); ZIGP_TRY(tap->snap(c, tf.P, jb.P, mq * mq)); ZIGP_TRY(tap->snap(c, tf.PF, jb.PF, mq * mq));
        ZIGP_TRY(tap->snap(c, tf.dvec, jb.dvec, mq + 1)); ZIGP_TRY(tap->snap(c, tf.Zs, jb.Zs, mq * jb.D)); ZIGP_TRY(tap->snap(c, tf.zc, jb.zc_out, (size_t)jb.D));
      }
  }
  return 0;
}

template <bool TAP>
static int kf_stage_latent(KfRun& s, KfTap* tap) {
  zigp_ctx* c = s.c;
  KfLatentArgs la;
  memset(&la, 0, sizeof(la));
  for (int h = 0; h < s.nlat; ++h) {
    KfLatentJob& jb = la.job[h];
    jb.M0 = s.k->hl[h].M[0]; jb.M1 = s.k->hl[h].M[1]; jb.Mq0 = s.Mq[h][0]; jb.Mq1 = s.Mq[h][1];
    jb.P0 = s.fac(h, 0) + s.FAC_P; jb.P1 = s.fac(h, 1) + s.FAC_P; jb.dvec0 = s.fac(h, 0) + s.FAC_DV; jb.dvec1 = s.fac(h, 1) + s.FAC_DV;
    jb.PF0 = s.fac(h, 0) + s.FAC_PF; jb.PF1 = s.fac(h, 1) + s.FAC_PF;
    jb.u = s.ks->in.p + s.off_u[h]; jb.s = s.ks->in.p + s.off_s[h];
    double* L = s.lat(h);
    jb.U = L + s.LAT_U; jb.S2 = L + s.LAT_S2; jb.T0 = L + s.LAT_T0; jb.T1 = L + s.LAT_T1; jb.Al = L + s.LAT_AL;
    jb.AlF = L + s.LAT_ALF; jb.S2F = L + s.LAT_S2F; jb.AlTF = L + s.LAT_ALTF; jb.S2TF = L + s.LAT_S2TF;
    jb.klv = s.res(h) + s.RES_KLV;
  }
  if (s.pl.large) {
    int mq1 = 0;
    for (int h = 0; h < s.nlat; ++h) mq1 = std::max(mq1, la.job[h].Mq1);
    hipLaunchKernelGGL(k_kfl_latent, dim3(s.nlat), dim3(1024), kfl_latent_lds(mq1), c->stream, la);
  }
  else hipLaunchKernelGGL(k_kf_latent, dim3(s.nlat), dim3(1024), 0, c->stream, la);
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) {
    for (int h = 0; h < s.nlat; ++h) {
      const zigp_kronf_tap_latent& tl = tap->s->lat[h];
      const KfLatentJob& jb = la.job[h];
      const size_t n01 = (size_t)jb.Mq0 * jb.Mq1;
      double* const host[9] = {tl.U, tl.S2, tl.T0, tl.T1, tl.Al, tl.AlF, tl.S2F, tl.AlTF, tl.S2TF};
      const double* const dev[9] = {jb.U, jb.S2, jb.T0, jb.T1, jb.Al, jb.AlF, jb.S2F, jb.AlTF, jb.S2TF};
      for (int i = 0; i < 9; ++i) ZIGP_TRY(tap->snap(c, host[i], dev[i], n01));
      ZIGP_TRY(tap->snap(c, tl.klv, jb.klv, 8));
    }
  }
  return 0;
}

// fills ka, the arguments the point kernels of the step share (the backward stage adds its accumulators), and launches the forward ones
template <bool TAP>
static int kf_stage_point_forward(KfRun& s, KfTap* tap, const double* Xd, KfArgs& ka) {
  zigp_ctx* c = s.c;
  const int nlat = s.nlat;
  const int64_t Npad = s.Npad;
  memset(&ka, 0, sizeof(ka));
  ka.X = Xd; ka.N = s.N; ka.Npad = Npad; ka.ldx = s.ldx; ka.ntiles = (int)(Npad / 16);
  for (int h = 0; h < nlat; ++h) {
    KfLat& L = ka.lat[h];
    for (int q = 0; q < 2; ++q) {
      KfFac& f = L.f[q];
      f.M = s.k->hl[h].M[q]; f.nb = s.Mq[h][q] / 16; f.D = q == 0 ? s.D0 : s.D1; f.col0 = q == 0 ? 0 : s.D0;
      f.hyp = s.d_hyp + (2 * h + q) * KH_FAC;
      f.Zs = s.fac(h, q) + s.FAC_ZS; f.PF = s.fac(h, q) + s.FAC_PF;
    }
    double* Lm = s.lat(h);
    L.AlF = Lm + s.LAT_ALF; L.S2F = Lm + s.LAT_S2F; L.AlTF = Lm + s.LAT_ALTF; L.S2TF = Lm + s.LAT_S2TF;
    double* P = s.pts(h);
    L.part = P; L.gm = P + 4 * Npad; L.gv = P + 5 * Npad; L.dq0 = P + 6 * Npad; L.dq1 = P + 7 * Npad;
  }
  const int waves = std::min(ka.ntiles, s.pl.large ? 1024 / nlat : 2048);
  ka.tpw = (ka.ntiles + waves - 1) / waves;
  const int nw = (ka.ntiles + ka.tpw - 1) / ka.tpw;
  const dim3 grid((nw + KF_WAVES - 1) / KF_WAVES, nlat);
  if (s.pl.large && s.kinds) {
    if (s.large_exact) hipLaunchKernelGGL((k_kfl_forward_kinds<1, 7, true, true>), grid, dim3(64 * KF_WAVES), s.lds_fwd, c->stream, ka, s.kinds);
    else hipLaunchKernelGGL((k_kfl_forward_kinds<1, 7, true, false>), grid, dim3(64 * KF_WAVES), s.lds_fwd, c->stream, ka, s.kinds);
  }
  else if (s.pl.large && s.large_exact) hipLaunchKernelGGL((k_kfl_forward<1, 7, true, true>), grid, dim3(64 * KF_WAVES), s.lds_fwd, c->stream, ka);
  else if (s.pl.large) hipLaunchKernelGGL((k_kfl_forward<1, 7, true, false>), grid, dim3(64 * KF_WAVES), s.lds_fwd, c->stream, ka);
  else ZIGP_TRY(kf_launch_small_latents(c, s.Mq, nlat, false, grid.x, ka, s.kinds));
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) {
    tap->facts[ZIGP_KFF_TPW_FWD] = ka.tpw;
    for (int h = 0; h < nlat; ++h) ZIGP_TRY(tap->snap(c, tap->s->lat[h].part, s.pts(h), (size_t)4 * Npad));
  }
  return 0;
}

// the point-wise kernel: a prediction ends with it (rows -> KfState::out); a value-only step adds the sum of its block partials
template <bool TAP>
static int kf_stage_pointwise(KfRun& s, KfTap* tap, const double* Yd) {
  zigp_ctx* c = s.c;
  KfState& ks = *s.ks;
  const KronCall& k = *s.k;
  const int nlat = s.nlat, pw_blocks = s.pw_blocks;
  const int64_t N = s.N, Npad = s.Npad;
  KronPwArgs a;
  memset(&a, 0, sizeof(a));
  const int gl_ = nlat - 1;   // latent whose buffers stand in for g (unused by the single-latent kernels)
  a.part_f = s.pts(0); a.part_g = s.pts(gl_); a.Y = Yd; a.N = N; a.Nc = Npad;
  a.hyp = s.d_hyp;            // knn_f, knn_g, noise: from the device block (the single-latent heads outside a fit call read the by-value fields below)
  if (!s.fit) { a.knn_f = k.p->var0f * k.p->var1f; a.knn_g = k.p->var0g * k.p->var1g; a.noise = k.p->noise; }
  a.g_offset = k.g_offset; a.f_offset = k.f_mu; a.scale = k.scale;
  a.gm_f = s.need_grad ? s.pts(0) + 4 * Npad : nullptr; a.gv_f = s.pts(0) + 5 * Npad; a.gm_g = s.pts(gl_) + 4 * Npad; a.gv_g = s.pts(gl_) + 5 * Npad;
  a.dq0_f = s.pts(0) + 6 * Npad; a.dq1_f = s.pts(0) + 7 * Npad; a.dq0_g = s.pts(gl_) + 6 * Npad; a.dq1_g = s.pts(gl_) + 7 * Npad;
  a.acc = s.d_pwacc; a.out9 = nullptr; a.ld9 = N;
  if (k.predict) {
    const int rows = nlat == 2 ? 9 : 4;
    ZIGP_ENSURE(c, ks.out, (size_t)rows * N);
    a.out9 = ks.out.p;
    if (nlat == 2) hipLaunchKernelGGL(k_kron_pointwise<true>, dim3(pw_blocks), dim3(PW_THREADS), 0, c->stream, a);
    else hipLaunchKernelGGL((k_kron_head_pointwise<true, false>), dim3(pw_blocks), dim3(PW_THREADS), 0, c->stream, a, k.lik);
    ZIGP_HIP(c, hipGetLastError());
    return 0;
  }
  if (nlat == 2) hipLaunchKernelGGL(k_kron_pointwise<false>, dim3(pw_blocks), dim3(PW_THREADS), 0, c->stream, a);
  else if (s.fit) hipLaunchKernelGGL((k_kron_head_pointwise<false, true>), dim3(pw_blocks), dim3(PW_THREADS), 0, c->stream, a, k.lik);   // Knn, noise, f_mu: device block
  else hipLaunchKernelGGL((k_kron_head_pointwise<false, false>), dim3(pw_blocks), dim3(PW_THREADS), 0, c->stream, a, k.lik);
  if (!s.need_grad) hipLaunchKernelGGL(k_kron_pw_reduce, dim3(1), dim3(256), 0, c->stream, s.d_pwacc, pw_blocks, k.include_kl ? 1.0 : 0.0, ks.res.p + s.RES_PWS);
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) {
    for (int h = 0; h < nlat; ++h) {
      ZIGP_TRY(tap->snap(c, tap->s->lat[h].cot, s.pts(h) + 4 * Npad, (size_t)4 * Npad));
      if (tap->s->lat[h].inject)      // rows [4][N] over gm, gv, dq0, dq1 [Npad] each: the padding keeps the kernel's values
        ZIGP_HIP(c, hipMemcpy2DAsync(s.pts(h) + 4 * Npad, sizeof(double) * Npad, tap->inject[h].p, sizeof(double) * N, sizeof(double) * N, 4,
                                     hipMemcpyDeviceToDevice, c->stream));
    }
  }
  return 0;
}

// small grid: the accumulators stay in registers, one partial per wave (nparts of them)
template <bool TAP>
static int kf_stage_backward_small(KfRun& s, KfTap* tap, KfArgs& ka, int& nparts) {
  zigp_ctx* c = s.c;
  KfState& ks = *s.ks;
  const int waves = std::min(ka.ntiles, 1024 / s.nlat);   // one wave per SIMD of the chip: the kernels hold ~400-500 registers per lane
  ka.tpw = (ka.ntiles + waves - 1) / waves;
  const int nw = (ka.ntiles + ka.tpw - 1) / ka.tpw;
  const int nwg = (nw + KF_WAVES - 1) / KF_WAVES;
  nparts = nwg * KF_WAVES;
  ZIGP_ENSURE(c, ks.acc, (size_t)2 * nparts * s.nblk * 256);
  for (int h = 0; h < s.nlat; ++h) ka.lat[h].acc = ks.acc.p + (size_t)h * nparts * s.nblk * 256;
  ZIGP_TRY(kf_launch_small_latents(c, s.Mq, s.nlat, true, (unsigned)nwg, ka, s.kinds));
  if constexpr (TAP) { tap->facts[ZIGP_KFF_TPW_BWD] = ka.tpw; tap->facts[ZIGP_KFF_NRANGES] = 1; }
  return 0;
}

// The larger-grid backward kernel spills ~4 KB of operands per point and latent (at 10 x 100), which k_kfl_accum then sums over the points.
// The rows go through in RANGES of <= 1024 tiles (16 384 rows: <= 128 MB of records for both latents, Infinity-Cache resident), one
// backward + one accumulate launch per range.  The split of the tiles into accumulation parts of tps tiles does not depend on the
// ranges (a range is a whole number of parts), so the partial sums -- and k_kf_reduce's fixed-order total -- are the same bits as
// with one range over everything; memory no longer grows with the row count (rounds 2-3: 0.86 GB for the pptr full batch, and a
// 64 GB cap with an error beyond it).
template <bool TAP>
static int kf_stage_backward_large(KfRun& s, KfTap* tap, KfArgs& ka, int& nparts) {
  zigp_ctx* c = s.c;
  KfState& ks = *s.ks;
  const int nlat = s.nlat, nblk = s.nblk;
  size_t rec[2] = {0, 0};
  for (int h = 0; h < nlat; ++h) rec[h] = (size_t)(s.kinds ? 80 : 64) * (s.Mq[h][0] + s.Mq[h][1]);      // _kinds: t'_0 | t'_1 behind the eight images
  const int tps = std::max(4, std::min(64, ka.ntiles / 16));     // tiles per accumulation part (4 for a minibatch: the chain of dependent loads is short)
  nparts = (ka.ntiles + tps - 1) / tps;
  const int range_tiles = std::max(1, c->kron_range_tiles / tps) * tps;
  const int spill_tiles = std::min(ka.ntiles, range_tiles);
  ZIGP_ENSURE(c, ks.spill, (rec[0] + (nlat == 2 ? rec[1] : 0)) * spill_tiles);
  ka.lat[0].spill = ks.spill.p;
  if (nlat == 2) ka.lat[1].spill = ks.spill.p + rec[0] * spill_tiles;
  ZIGP_ENSURE(c, ks.acc, (size_t)2 * nparts * nblk * 256);
  KflAccArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.X = ka.X; aa.N = s.N; aa.ldx = s.ldx; aa.ntiles = ka.ntiles; aa.tps = tps; aa.nb0c = s.pl.nb0c; aa.nb1c = s.pl.nb1c;
  for (int h = 0; h < nlat; ++h) {
    KflAccLat& L = aa.lat[h];
    L.spill = ka.lat[h].spill; L.gm = ka.lat[h].gm; L.gv = ka.lat[h].gv;
    L.acc = ks.acc.p + (size_t)h * nparts * nblk * 256;
    ka.lat[h].acc = L.acc;
    L.nb0 = s.Mq[h][0] / 16; L.nb1 = s.Mq[h][1] / 16; L.D0 = s.D0; L.D1 = s.D1;
    L.hyp0 = s.d_hyp + (2 * h) * KH_FAC; L.hyp1 = s.d_hyp + (2 * h + 1) * KH_FAC;
  }
  for (int t0 = 0; t0 < ka.ntiles; t0 += range_tiles) {
    const int t1 = std::min(t0 + range_tiles, ka.ntiles), nt = t1 - t0;
    const int rwaves = std::min(nt, 1024 / nlat);   // one wave per SIMD of the chip: the kernels hold ~400-500 registers per lane
    ka.tile0 = t0; ka.tile1 = t1; ka.tpw = (nt + rwaves - 1) / rwaves;
    const int rnw = (nt + ka.tpw - 1) / ka.tpw, rnwg = (rnw + KF_WAVES - 1) / KF_WAVES;
    if (s.kinds) {
      if (s.large_exact) hipLaunchKernelGGL((k_kfl_backward_kinds<1, 7, true, true>), dim3(rnwg, nlat), dim3(64 * KF_WAVES), s.lds_bwd, c->stream, ka, s.kinds);
      else hipLaunchKernelGGL((k_kfl_backward_kinds<1, 7, true, false>), dim3(rnwg, nlat), dim3(64 * KF_WAVES), s.lds_bwd, c->stream, ka, s.kinds);
    }
    else if (s.large_exact) hipLaunchKernelGGL((k_kfl_backward<1, 7, true, true>), dim3(rnwg, nlat), dim3(64 * KF_WAVES), s.lds_bwd, c->stream, ka);
    else hipLaunchKernelGGL((k_kfl_backward<1, 7, true, false>), dim3(rnwg, nlat), dim3(64 * KF_WAVES), s.lds_bwd, c->stream, ka);
    ZIGP_HIP(c, hipGetLastError());
    aa.tile0 = t0; aa.tile1 = t1; aa.part0 = t0 / tps;
    if (s.kinds) hipLaunchKernelGGL(k_kfl_accum_kinds, dim3((nblk + 3) / 4, (nt + tps - 1) / tps, nlat), dim3(256), 0, c->stream, aa, s.kinds);
    else hipLaunchKernelGGL(k_kfl_accum, dim3((nblk + 3) / 4, (nt + tps - 1) / tps, nlat), dim3(256), 0, c->stream, aa);
    ZIGP_HIP(c, hipGetLastError());
    if constexpr (TAP) { if (t0 == 0) tap->facts[ZIGP_KFF_TPW_BWD] = ka.tpw; ++tap->facts[ZIGP_KFF_NRANGES]; }
  }
  if constexpr (TAP) { tap->facts[ZIGP_KFF_TPS] = tps; tap->facts[ZIGP_KFF_RANGE_TILES] = range_tiles; }
  return 0;
}

// fixed-order sum of the nparts partials into the work buffers; its extra workgroup sums the point-wise block partials (k_kron_pw_reduce)
template <bool TAP>
static int kf_stage_reduce(KfRun& s, KfTap* tap, const KfArgs& ka, int nparts) {
  zigp_ctx* c = s.c;
  const int nlat = s.nlat, gl_ = nlat - 1;
  hipLaunchKernelGGL(k_kf_reduce, dim3(s.nblk * 256 / 16 + 1, nlat), dim3(256), 0, c->stream, ka.lat[0].acc, ka.lat[gl_].acc, nparts,
                     s.lat(0) + s.LAT_WORK, s.lat(gl_) + s.LAT_WORK, s.pl.nb0c, s.pl.nb1c, s.Mq[0][0] / 16, s.Mq[0][1] / 16, s.Mq[gl_][0] / 16, s.Mq[gl_][1] / 16,
                     s.d_pwacc, s.pw_blocks, s.k->include_kl ? 1.0 : 0.0, s.ks->res.p + s.RES_PWS);
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) {
    tap->facts[ZIGP_KFF_NPARTS] = nparts;
    for (int h = 0; h < nlat; ++h) ZIGP_TRY(tap->snap(c, tap->s->lat[h].work, s.lat(h) + s.LAT_WORK, (size_t)s.wl.total));
  }
  return 0;
}

// work buffers -> the result block: krow of both factors, the gradients of u and s
template <bool TAP>
static int kf_stage_finish(KfRun& s, KfTap* tap) {
  zigp_ctx* c = s.c;
  const int nlat = s.nlat;
  const KfWork& wl = s.wl;
  // the krow regions of the result block at their capacity sizes (kf_prepare: RES_KROW0 .. RES_GU)
  const size_t n_krow[2] = {s.RES_KROW1 - s.RES_KROW0, s.RES_GU - s.RES_KROW1};
  KflFinishArgs fa;
  memset(&fa, 0, sizeof(fa));
  for (int h = 0; h < nlat; ++h) {
    KfFinishJob& jb = fa.job[h];
    jb.M0 = s.k->hl[h].M[0]; jb.M1 = s.k->hl[h].M[1]; jb.Mq0 = s.Mq[h][0]; jb.Mq1 = s.Mq[h][1]; jb.D0 = s.D0; jb.D1 = s.D1;
    jb.P0 = s.fac(h, 0) + s.FAC_P; jb.P1 = s.fac(h, 1) + s.FAC_P; jb.dvec0 = s.fac(h, 0) + s.FAC_DV; jb.dvec1 = s.fac(h, 1) + s.FAC_DV;
    jb.PF0 = s.fac(h, 0) + s.FAC_PF; jb.PF1 = s.fac(h, 1) + s.FAC_PF;
    jb.K0 = s.fac(h, 0); jb.K1 = s.fac(h, 1); jb.Z0 = s.ks->in.p + s.off_z[h][0]; jb.Z1 = s.ks->in.p + s.off_z[h][1];
    jb.hyp0 = s.d_hyp + (2 * h) * KH_FAC; jb.hyp1 = s.d_hyp + (2 * h + 1) * KH_FAC;
    double* L = s.lat(h);
    jb.U = L + s.LAT_U; jb.S2 = L + s.LAT_S2; jb.T0 = L + s.LAT_T0; jb.T1 = L + s.LAT_T1; jb.Al = L + s.LAT_AL; jb.s = s.ks->in.p + s.off_s[h];
    jb.work = L + s.LAT_WORK;
    jb.krow0 = s.res(h) + s.RES_KROW0; jb.krow1 = s.res(h) + s.RES_KROW1; jb.gu = s.res(h) + s.RES_GU; jb.gs = s.res(h) + s.RES_GS;
  }
  fa.jitter = s.k->jitter; fa.with_kl = s.k->include_kl ? 1 : 0;
  fa.ldw = wl.ldw; fa.wS2 = wl.S2; fa.wP0 = wl.P0; fa.wP1 = wl.P1; fa.wK0 = wl.K0; fa.wK1 = wl.K1;
  fa.scratch_off = (int64_t)wl.total; fa.scratch_set = (int64_t)s.SCR_SET;
  if (s.pl.large) {
    int nbmax = 1;
    for (int h = 0; h < nlat; ++h) nbmax = std::max(nbmax, std::max(s.Mq[h][0], s.Mq[h][1]) / 16);
    const dim3 grid(nbmax, 2, nlat);
    if constexpr (TAP) {      // the regions stage 3 leaves its G rows in hold the stage sentinel before stage 1: what comes back as the sentinel was never written
      const size_t rmax = (size_t)wl.ldw * wl.ldw;
      for (int h = 0; h < nlat; ++h)
        for (int q = 0; q < 2; ++q)
          if (tap->s->lat[h].G[q]) ZIGP_HIP(c, hipMemsetAsync(s.lat(h) + s.LAT_SCR + (size_t)q * s.SCR_SET + 2 * rmax, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * rmax, c->stream));
    }
    hipLaunchKernelGGL(k_kfl_finish<1>, grid, dim3(KFL_FIN_THREADS), 0, c->stream, fa);
    hipLaunchKernelGGL(k_kfl_finish<2>, grid, dim3(KFL_FIN_THREADS), 0, c->stream, fa);
    hipLaunchKernelGGL(k_kfl_finish<3>, grid, dim3(KFL_FIN_THREADS), 0, c->stream, fa);
    if constexpr (TAP) {      // stage 3's G rows (the Q region of the factor's scratch set), and the krow rows k_kfl_krow_kinds is about to rewrite
      ZIGP_HIP(c, hipGetLastError());
      const size_t rmax = (size_t)wl.ldw * wl.ldw;
      for (int h = 0; h < nlat; ++h) {
        const zigp_kronf_tap_latent& tl = tap->s->lat[h];
        for (int q = 0; q < 2; ++q) {
          ZIGP_TRY(tap->snap(c, tl.G[q], s.lat(h) + s.LAT_SCR + (size_t)q * s.SCR_SET + 2 * rmax, rmax));
          if (s.kinds) ZIGP_TRY(tap->snap(c, tl.krow_first[q], q == 0 ? fa.job[h].krow0 : fa.job[h].krow1, n_krow[q]));
        }
      }
    }
    if (s.kinds) hipLaunchKernelGGL(k_kfl_krow_kinds, grid, dim3(KFL_FIN_THREADS), 0, c->stream, fa, s.kinds);      // the krow rows of the Matern factors
  } else {
    KfFinishArgs fs;
    memset(&fs, 0, sizeof(fs));
    fs.job[0] = fa.job[0]; fs.job[1] = fa.job[1]; fs.jitter = fa.jitter; fs.with_kl = fa.with_kl;
    hipLaunchKernelGGL(k_kf_finish, dim3(2, nlat), dim3(1024), KF_FIN_LDS, c->stream, fs);
    if (s.kinds) {      // Matern factors: the second run on K' and sum t' (k_kf_kd_prepare), then the merge of its moment columns
      ZIGP_HIP(c, hipGetLastError());
      ZIGP_ENSURE(c, s.ks->spill, (size_t)2 * KF_KD_TOTAL);
      KfKdArgs ka;
      memset(&ka, 0, sizeof(ka));
      KfFinishArgs f2 = fs;
      for (int h = 0; h < nlat; ++h) {
        const KfFinishJob& jb = fs.job[h];
        KfKdJob& kj = ka.job[h];
        double* buf = s.ks->spill.p + (size_t)h * KF_KD_TOTAL;
        kj.M0 = jb.M0; kj.M1 = jb.M1; kj.D0 = jb.D0; kj.D1 = jb.D1; kj.Z0 = jb.Z0; kj.Z1 = jb.Z1; kj.hyp0 = jb.hyp0; kj.hyp1 = jb.hyp1;
        kj.work = jb.work; kj.buf = buf; kj.krow0 = jb.krow0; kj.krow1 = jb.krow1;
        KfFinishJob& j2 = f2.job[h];
        if (kf_kind_of(s.kinds, h, 0) != KERN_RBF) j2.K0 = buf;
        if (kf_kind_of(s.kinds, h, 1) != KERN_RBF) j2.K1 = buf + KF_KD_K;
        j2.work = buf + KF_KD_WORK; j2.krow0 = buf + KF_KD_KROW0; j2.krow1 = buf + KF_KD_KROW1; j2.gu = buf + KF_KD_GU; j2.gs = buf + KF_KD_GS;
      }
      if constexpr (TAP) {    // the first run's krow; the second run's scratch (K' images, work', krow', gu', gs') holds the stage sentinel wherever its kernels do not write (nothing reads it there)
        for (int h = 0; h < nlat; ++h) {
          const zigp_kronf_tap_latent& tl = tap->s->lat[h];
          ZIGP_TRY(tap->snap(c, tl.krow_first[0], fs.job[h].krow0, n_krow[0])); ZIGP_TRY(tap->snap(c, tl.krow_first[1], fs.job[h].krow1, n_krow[1]));
          if (tl.Kd[0] || tl.Kd[1] || tl.krow2[0] || tl.krow2[1]) ZIGP_HIP(c, hipMemsetAsync(ka.job[h].buf, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * KF_KD_TOTAL, c->stream));
        }
      }
      hipLaunchKernelGGL(k_kf_kd_prepare, dim3(3, nlat), dim3(256), 0, c->stream, ka, s.kinds);
      if constexpr (TAP) {
        ZIGP_HIP(c, hipGetLastError());
        for (int h = 0; h < nlat; ++h) {
          const zigp_kronf_tap_latent& tl = tap->s->lat[h];
          ZIGP_TRY(tap->snap(c, tl.Kd[0], ka.job[h].buf, (size_t)KF_KD_K)); ZIGP_TRY(tap->snap(c, tl.Kd[1], ka.job[h].buf + KF_KD_K, (size_t)KF_KD_K));
          ZIGP_TRY(tap->snap(c, tl.work2, ka.job[h].buf + KF_KD_WORK, (size_t)KF_W_TOTAL));
        }
      }
      hipLaunchKernelGGL(k_kf_finish, dim3(2, nlat), dim3(1024), KF_FIN_LDS, c->stream, f2);
      if constexpr (TAP) {
        ZIGP_HIP(c, hipGetLastError());
        for (int h = 0; h < nlat; ++h) {
          const zigp_kronf_tap_latent& tl = tap->s->lat[h];
          ZIGP_TRY(tap->snap(c, tl.krow2[0], f2.job[h].krow0, (size_t)KF_KD_KROW1 - KF_KD_KROW0)); ZIGP_TRY(tap->snap(c, tl.krow2[1], f2.job[h].krow1, (size_t)KF_KD_GU - KF_KD_KROW1));
        }
      }
      hipLaunchKernelGGL(k_kf_krow_merge, dim3(2, nlat), dim3(256), 0, c->stream, ka, s.kinds);
    }
  }
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) {        // what the LAST launch of the stage leaves in the result block
    for (int h = 0; h < nlat; ++h) {
      const zigp_kronf_tap_latent& tl = tap->s->lat[h];
      ZIGP_TRY(tap->snap(c, tl.krow[0], fa.job[h].krow0, n_krow[0])); ZIGP_TRY(tap->snap(c, tl.krow[1], fa.job[h].krow1, n_krow[1]));
      ZIGP_TRY(tap->snap(c, tl.gu, fa.job[h].gu, s.RES_GS - s.RES_GU)); ZIGP_TRY(tap->snap(c, tl.gs, fa.job[h].gs, s.RES_SIZE - s.RES_GS));
    }
  }
  return 0;
}

template <bool TAP>
static int kf_step(KfRun& s, KfTap* tap, const double* Xd, const double* Yd) {
  zigp_ctx* c = s.c;
  const bool predict = s.k->predict;
  if (c->comm && !predict) ZIGP_HIP(c, hipMemsetAsync(s.ks->res.p, 0, sizeof(double) * s.RES_INFO, c->stream));   // parts a value-only / single-latent step leaves unwritten
  if constexpr (TAP) {      // the stage tests see what a step does NOT write: the latents' result blocks hold the stage sentinel first (nothing reads an
    // unwritten part: kf_gather takes klv[0..4] and the compact krow, gu, gs).  A data-parallel step has just cleared the block instead: +0 there.
    bool wanted = false;      // a step with none of these taps enqueues nothing
    for (int h = 0; h < s.nlat; ++h) {
      const zigp_kronf_tap_latent& tl = tap->s->lat[h];
      wanted = wanted || tl.klv || tl.krow[0] || tl.krow[1] || tl.gu || tl.gs || tl.krow_first[0] || tl.krow_first[1];
    }
    if (wanted && !c->comm && !predict) ZIGP_HIP(c, hipMemsetAsync(s.ks->res.p, ZIGP_STAGE_SENTINEL_BYTE, sizeof(double) * s.nlat * s.RES_SIZE, c->stream));
  }
  ZIGP_TRY(kf_stage_factor<TAP>(s, tap));
  if (predict) ZIGP_TRY(request_info(c, &s.hinfo));   // value / gradient steps: the status slots come back with the result block
  ZIGP_TRY(kf_stage_latent<TAP>(s, tap));
  KfArgs ka;
  ZIGP_TRY(kf_stage_point_forward<TAP>(s, tap, Xd, ka));
  ZIGP_TRY(kf_stage_pointwise<TAP>(s, tap, Yd));
  if (predict) return 0;
  if (s.need_grad) {
    int nparts = 0;
    if (s.pl.large) ZIGP_TRY(kf_stage_backward_large<TAP>(s, tap, ka, nparts));
    else ZIGP_TRY(kf_stage_backward_small<TAP>(s, tap, ka, nparts));
    ZIGP_TRY(kf_stage_reduce<TAP>(s, tap, ka, nparts));
    ZIGP_TRY(kf_stage_finish<TAP>(s, tap));
  }
  if (c->comm) {   // data-parallel run: the block (cleared at the start of the step) is summed over ranks where it lies
    // a rank that does not count the KL (include_kl = 0) must not add its scalars, which the latent kernel writes regardless
    if (!s.k->include_kl) for (int h = 0; h < s.nlat; ++h) ZIGP_HIP(c, hipMemsetAsync(s.res(h) + s.RES_KLV, 0, sizeof(double) * 8, c->stream));
    ZIGP_TRY(comm_allreduce(c, s.ks->res.p, s.RES_INFO));
  }
  return 0;
}

// the plan of the step as the stage tests read it (ZIGP_KFF_*); the stages fill in the launch facts
static void kf_tap_plan(const KfRun& s, KfTap* tap) {
  const int g = s.nlat - 1;
  const int64_t f0[ZIGP_KFF_COUNT] = {s.pl.large, s.large_exact, s.pl.nb0c, s.pl.nb1c, s.Mq[0][0] / 16, s.Mq[0][1] / 16, s.Mq[g][0] / 16, s.Mq[g][1] / 16,
                                      s.Npad, s.Npad / 16, 0, 0, 0, 0, 0, 0,
                                      (s.pl.large || s.nlat == 1 || (s.Mq[0][0] == s.Mq[1][0] && s.Mq[0][1] == s.Mq[1][1])) ? 1 : 0};
  memcpy(tap->facts, f0, sizeof(f0));
}

// ---- fit call: n_steps steps back to back, parameters updated on the device, ONE synchronisation at the end ----
// the descriptor of k_fit_update: the blocks of the free vector, where their values go in the parameter image, the result block
static int kf_fit_describe(const KfRun& s, KfFitDesc& d) {
  const KfFitCall* fit = s.fit;
  const int nlat = s.nlat;
  d.nlat = nlat; d.D0 = s.D0; d.D1 = s.D1;
  const int nblocks = fit->head ? ZIGP_HEAD_FIT_BLOCKS : KFIT_BLOCKS;
  size_t o = 0;
  auto block = [&](int b, int n, size_t dst) {
    d.off[b] = (int)o; d.n[b] = n; d.dst[b] = (int)dst; d.positive[b] = fit->positive[b]; d.lr[b] = fit->lr[b];
    d.trainable[b] = fit->trainable ? (fit->trainable[b] != 0) : 1;
    o += n;
  };
  for (int h = 0; h < nlat; ++h) {
    const int M0 = s.k->hl[h].M[0], M1 = s.k->hl[h].M[1];
    const int sizes[8] = {M0 * s.D0, M1 * s.D1, M0 * M1, M0 * M1, s.D0, s.D1, 1, 1};
    const size_t dsts[8] = {s.off_z[h][0], s.off_z[h][1], s.off_u[h], s.off_s[h], 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) block(8 * h + k, sizes[k], dsts[k]);
    for (int q = 0; q < 2; ++q) { d.M[h][q] = s.k->hl[h].M[q]; d.Mq[h][q] = s.Mq[h][q]; d.off_z[h][q] = (int)s.off_z[h][q]; }
  }
  for (int b = 8 * nlat; b < nblocks; ++b) block(b, 1, 0);      // the likelihood variance (head: and f_mu)
  if ((int64_t)o != fit->n_free) { s.c->err = std::string(fit->name) + ": n_free does not match the model sizes"; return ZIGP_EARG; }
  d.off_hyp = (int)s.off_hyp; d.off_hyp2 = (int)s.off_hyp2;
  int nbig = 0, nhyp = 0, kb = 0, kh = 0;
  for (int b = 0; b < nblocks; ++b) {
    const bool big = b < 8 * nlat && b % 8 <= 3;
    if (big) { d.big_blk[kb] = b; d.big_off[kb++] = nbig; nbig += d.n[b]; }
    else { d.hyp_blk[kh] = b; d.hyp_off[kh++] = nhyp; nhyp += d.n[b]; }
  }
  for (; kb <= 8; ++kb) d.big_off[kb] = nbig;      // kfit_element walks eight big and nine hyperparameter blocks: the ones a
  for (; kh <= 9; ++kh) d.hyp_off[kh] = nhyp;      // layout does not have start at the total (no thread maps to them)
  d.res_size = (int)s.RES_SIZE; d.res_krow0 = (int)s.RES_KROW0; d.res_krow1 = (int)s.RES_KROW1; d.res_gu = (int)s.RES_GU; d.res_gs = (int)s.RES_GS;
  d.res_pws = (int)s.RES_PWS; d.res_info = (int)s.RES_INFO;
  d.beta1 = fit->beta1; d.beta2 = fit->beta2; d.eps = fit->eps;
  return 0;
}

// Test hook of the loop (zigp_test_kron_fit_update, include/zigp_diag.h): step i's result block comes from the caller, and the state and the
// parameter image are snapshot -- device-to-device, on the loop's stream -- behind the initial image launch and behind every update launch.
struct KfFitTap {
  const zigp_stage_kron_fit_update* s;
  DevBuf res, snaps;          // the caller's result blocks [n_steps][n_res]; snapshots [1 + n_steps][3 n_free + n_img]
  size_t nf, n_img;
  int taken;
  int64_t facts[ZIGP_KFU_COUNT];
  int snap(zigp_ctx* c, const double* state, const double* img) {
    double* q = snaps.p + (size_t)taken++ * (3 * nf + n_img);
    ZIGP_HIP(c, hipMemcpyAsync(q, state, sizeof(double) * 3 * nf, hipMemcpyDeviceToDevice, c->stream));
    ZIGP_HIP(c, hipMemcpyAsync(q + 3 * nf, img, sizeof(double) * n_img, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  int flush(zigp_ctx* c) {      // the stream is idle
    std::vector<double> h((size_t)taken * (3 * nf + n_img));
    if (!h.empty()) ZIGP_HIP(c, hipMemcpy(h.data(), snaps.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    double* const dst[3] = {s->snap_x, s->snap_m, s->snap_v};
    for (int k = 0; k < taken; ++k) {
      const double* q = h.data() + (size_t)k * (3 * nf + n_img);
      for (int j = 0; j < 3; ++j)
        if (dst[j]) memcpy(dst[j] + (size_t)k * nf, q + (size_t)j * nf, sizeof(double) * nf);
      if (s->snap_img) memcpy(s->snap_img + (size_t)k * n_img, q + 3 * nf, sizeof(double) * n_img);
    }
    return 0;
  }
};

template <bool TAP>
static int kf_fit_run(KfRun& s, KfFitTap* tap) {
  zigp_ctx* c = s.c;
  KfState& ks = *s.ks;
  const KfFitCall* fit = s.fit;
  const int64_t N = s.N;
  const int ldx = s.ldx;
  KfFitArgs fa;
  memset(&fa, 0, sizeof(fa));
  ZIGP_TRY(kf_fit_describe(s, fa.d));
  const KfFitDesc& d = fa.d;
  const size_t nf = (size_t)fit->n_free, n_hist = (size_t)2 * fit->n_steps;
  const size_t n_state = 3 * nf + n_hist + 8;
  if constexpr (TAP) {
    const zigp_stage_kron_fit_update* ts = tap->s;
    int64_t* f = tap->facts;
    const int64_t res[9] = {(int64_t)s.RES_KLV, (int64_t)s.RES_KROW0, (int64_t)s.RES_KROW1, (int64_t)s.RES_GU, (int64_t)s.RES_GS, (int64_t)s.RES_SIZE,
                            (int64_t)s.RES_PWS, (int64_t)s.RES_INFO, (int64_t)s.n_res};
    memcpy(f + ZIGP_KFU_RES_KLV, res, sizeof(res));
    f[ZIGP_KFU_GRID] = (d.big_off[8] + KFIT_THREADS - 1) / KFIT_THREADS + 1;
    for (int k = 0; k < 9; ++k) f[ZIGP_KFU_BIG_OFF + k] = d.big_off[k];
    for (int k = 0; k < 10; ++k) f[ZIGP_KFU_HYP_OFF + k] = d.hyp_off[k];
    f[ZIGP_KFU_N_IMG] = (int64_t)(s.off_hyp2 + KH_SIZE); f[ZIGP_KFU_OFF_HYP] = (int64_t)s.off_hyp; f[ZIGP_KFU_OFF_HYP2] = (int64_t)s.off_hyp2;
    for (int h = 0; h < 2; ++h) {
      for (int q = 0; q < 2; ++q) f[ZIGP_KFU_OFF_Z + 2 * h + q] = h < s.nlat ? (int64_t)s.off_z[h][q] : -1;
      f[ZIGP_KFU_OFF_U + h] = h < s.nlat ? (int64_t)s.off_u[h] : -1; f[ZIGP_KFU_OFF_S + h] = h < s.nlat ? (int64_t)s.off_s[h] : -1;
    }
    const int64_t kh[8] = {KH_SIZE, KH_FAC, KH_INV, KH_ZC, KH_ELL, KH_VAR, KH_NOISE, KH_FMU};
    memcpy(f + ZIGP_KFU_KH_SIZE, kh, sizeof(kh));
    if (ts->facts) memcpy(ts->facts, f, sizeof(tap->facts));
    if (!ts->res) return 0;       // the layout query
    if (ts->n_res != (int64_t)s.n_res || ts->n_img != f[ZIGP_KFU_N_IMG]) { c->err = "zigp_test_kron_fit_update: n_res / n_img differ from the facts"; return ZIGP_EARG; }
    tap->nf = nf; tap->n_img = (size_t)ts->n_img; tap->taken = 0;
    ZIGP_ENSURE(c, tap->res, (size_t)fit->n_steps * s.n_res);
    ZIGP_ENSURE(c, tap->snaps, (size_t)(1 + fit->n_steps) * (3 * nf + tap->n_img));
    ZIGP_HIP(c, hipMemcpyAsync(tap->res.p, ts->res, sizeof(double) * fit->n_steps * s.n_res, hipMemcpyHostToDevice, c->stream));
  }
  ZIGP_ENSURE(c, ks.fit, n_state);
  fa.x = ks.fit.p; fa.m = fa.x + nf; fa.v = fa.m + nf; fa.hist = fa.v + nf; fa.fail = reinterpret_cast<int*>(fa.hist + n_hist);
  fa.img = ks.in.p; fa.res = ks.res.p;
  {
    ZIGP_PINNED(c, hst, n_state);
    memcpy(hst, fit->x, sizeof(double) * nf); memcpy(hst + nf, fit->m, sizeof(double) * nf); memcpy(hst + 2 * nf, fit->v, sizeof(double) * nf);
    memset(hst + 3 * nf, 0, sizeof(double) * (n_hist + 8));
    ZIGP_HIP(c, hipMemcpyAsync(ks.fit.p, hst, sizeof(double) * n_state, hipMemcpyHostToDevice, c->stream));
    if (s.n_wrap) {
      const size_t nw = s.n_wrap * (size_t)N * (ldx + 1);
      ZIGP_PINNED(c, hw, nw);
      memcpy(hw, fit->Xw, sizeof(double) * s.n_wrap * N * ldx);
      memcpy(hw + s.n_wrap * (size_t)N * ldx, fit->Yw, sizeof(double) * s.n_wrap * N);
      ZIGP_HIP(c, hipMemcpyAsync(s.d_wrap, hw, sizeof(double) * nw, hipMemcpyHostToDevice, c->stream));
    }
  }
  ZIGP_HIP(c, hipMemsetAsync(ks.in.p + s.off_hyp, 0, sizeof(double) * 2 * KH_SIZE, c->stream));
  const dim3 ugrid((d.big_off[8] + KFIT_THREADS - 1) / KFIT_THREADS + 1);
  fa.update = 0; fa.step = 0;
  auto update = [&] {
    if (fit->head) hipLaunchKernelGGL(k_fit_update<true>, ugrid, dim3(KFIT_THREADS), 0, c->stream, fa);
    else hipLaunchKernelGGL(k_fit_update<false>, ugrid, dim3(KFIT_THREADS), 0, c->stream, fa);
  };
  update();       // free state -> parameter image (hyper block 0)
  ZIGP_HIP(c, hipGetLastError());
  if constexpr (TAP) ZIGP_TRY(tap->snap(c, ks.fit.p, ks.in.p));
  fa.update = 1;
  const double *X = s.k->X, *Y = s.k->Y;      // the resident data set
  for (int i = 0; i < fit->n_steps; ++i) {
    const int64_t rb = fit->row_begin[i];
    const double* Xd = rb >= 0 ? X + rb * ldx : s.d_wrap + (size_t)(-rb - 1) * N * ldx;
    const double* Yd = rb >= 0 ? Y + rb : s.d_wrap + s.n_wrap * (size_t)N * ldx + (size_t)(-rb - 1) * N;
    s.d_hyp = ks.in.p + ((i & 1) ? s.off_hyp2 : s.off_hyp);       // written by the previous step's update (step 0: by the launch above)
    if constexpr (TAP)      // the caller's result block in place of the step
      ZIGP_HIP(c, hipMemcpyAsync(ks.res.p, tap->res.p + (size_t)i * s.n_res, sizeof(double) * s.n_res, hipMemcpyDeviceToDevice, c->stream));
    else
      ZIGP_TRY(kf_step<false>(s, nullptr, Xd, Yd));
    // lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t counted from 1 (zigp/optim.py AdamGroups.step): the two t-dependent factors from the host
    const double t = (double)(fit->t0 + i + 1);
    fa.step = i; fa.lr_sq = std::sqrt(1.0 - std::pow(d.beta2, t)); fa.lr_den = 1.0 - std::pow(d.beta1, t);
    update();
    ZIGP_HIP(c, hipGetLastError());
    if constexpr (TAP) ZIGP_TRY(tap->snap(c, ks.fit.p, ks.in.p));
  }
  double* hst = nullptr;
  ZIGP_TRY(download(c, ks.fit.p, n_state, &hst));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  const int* hfail = reinterpret_cast<const int*>(hst + 3 * nf + n_hist);
  if constexpr (TAP) {
    if (tap->s->hist) memcpy(tap->s->hist, hst + 3 * nf, sizeof(double) * n_hist);
    if (tap->s->fail) memcpy(tap->s->fail, hfail, sizeof(int) * 4);
    ZIGP_TRY(tap->flush(c));
  }
  memcpy(fit->x, hst, sizeof(double) * nf); memcpy(fit->m, hst + nf, sizeof(double) * nf); memcpy(fit->v, hst + 2 * nf, sizeof(double) * nf);
  const int done = hfail[0] ? hfail[0] - 1 : fit->n_steps;       // steps whose update was applied
  c->fit_steps_applied = done;                                   // (zigp_kron_fit_steps_applied: the caller's iteration count advances by this)
  for (int i = 0; i < fit->n_steps; ++i) {
    if (fit->hist_data) fit->hist_data[i] = i < done ? hst[3 * nf + 2 * i] : NAN;
    if (fit->hist_kl) fit->hist_kl[i] = i < done ? hst[3 * nf + 2 * i + 1] : NAN;
  }
  if (hfail[0]) {
    char b[288];
    snprintf(b, sizeof(b), "Cholesky failed in step %d of this %s call (iteration %lld): %s not positive definite at pivot %d; "
             "the state returned is the one before that step", hfail[0] - 1, fit->name, (long long)(fit->t0 + hfail[0] - 1), kron_fac_names[hfail[1] & 3], hfail[2]);
    c->err = b; c->info = hfail[2];
    return ZIGP_ENOTPD;
  }
  return 0;
}

// the result block of a value / gradient step -> the outputs of the call
static int kf_gather(KfRun& s) {
  zigp_ctx* c = s.c;
  const KronCall& k = *s.k;
  double* hres = nullptr;
  ZIGP_TRY(download(c, s.ks->res.p, s.n_res, &hres));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < 2 * s.nlat; ++j) ZIGP_TRY(info_result(c, reinterpret_cast<const int*>(hres + s.RES_INFO) + 2 * j, kron_fac_names[j]));
  const double* pws = hres + s.RES_PWS;   // var_exp, d noise, sum gv_f, sum gv_g, sum gm_f (= d / d f_mu); [7]: the ranks that count the KL
  if (k.elbo_data) *k.elbo_data = pws[0];
  if (k.d_offset) *k.d_offset = pws[4];
  double* R[2] = {hres, hres + s.RES_SIZE};
  if (k.kl) { const double* klv[2] = {R[0] + s.RES_KLV, R[1] + s.RES_KLV}; *k.kl = kron_kl(k, klv, pws[7]); }
  if (s.need_grad) {
    double* krow[2][2] = {{R[0] + s.RES_KROW0, R[0] + s.RES_KROW1}, {R[1] + s.RES_KROW0, R[1] + s.RES_KROW1}};
    double* gu[2] = {R[0] + s.RES_GU, R[1] + s.RES_GU};
    double* gs[2] = {R[0] + s.RES_GS, R[1] + s.RES_GS};
    kron_assemble_grads(k, krow, gu, gs, pws + 2, pws[1]);
  }
  return 0;
}

// One ELBO step (or prediction) of the fused Kronecker path.  fit != nullptr: n_steps gradient steps with the Adam update on the device
// (k.p then carries the sizes only; k.X / k.Y are the resident data set).  tap != nullptr: the step of the stage tests
// (zigp_test_kron_fused_step).  fit_tap != nullptr: the fit loop of zigp_test_kron_fit_update.
static int kronf_run(zigp_ctx* c, const KronCall& k, const KfFitCall* fit = nullptr, KfTap* tap = nullptr, KfFitTap* fit_tap = nullptr) {
  KfRun s;
  ZIGP_TRY(kf_prepare(c, k, fit, s));
  if (!fit) ZIGP_TRY(kf_stage_inputs(s));
  if (k.predict) ZIGP_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
  ZIGP_TRY(kf_set_attributes(c));
  if (fit) return fit_tap ? kf_fit_run<true>(s, fit_tap) : kf_fit_run<false>(s, nullptr);
  const double* Xd = k.dev_xy ? k.X : s.ks->in.p + s.off_x;
  const double* Yd = k.Y ? (k.dev_xy ? k.Y : s.ks->in.p + s.off_y) : nullptr;
  if (tap) {
    kf_tap_plan(s, tap);
    ZIGP_TRY(kf_step<true>(s, tap, Xd, Yd));
  } else {
    ZIGP_TRY(kf_step<false>(s, nullptr, Xd, Yd));
  }
  if (!k.predict) return kf_gather(s);
  ZIGP_HIP(c, hipMemcpyAsync(k.out, s.ks->out.p, sizeof(double) * (k.nlat == 2 ? 9 : 4) * k.N, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return info_result(c, s.hinfo, kron_fac_any);
}

}  // namespace zigp
