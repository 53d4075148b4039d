// Sample-path scores: group totals, their CRPS, the energy score, the variogram score and the distance matrix of an ensemble against
// an observation (include/zigp_ensemble.h holds the definition).
//
// Members: P = S + 1, member S = the observation; padded to PP = 4 nb members (nb = ceil(P / 4) blocks of four; padding members are
// zero rows whose results nobody reads).  Rows of a group are taken in chunks of ENS_CH = 64 rows counted FROM THE GROUP'S START; chunk
// c of the call belongs to group g with cstart[g] <= c < cstart[g+1] (binary search over the G + 1 chunk prefix counts).
//
// k_ens_pairs<WEIGHTED>, one workgroup per chunk: the chunk's rows of all PP members go to LDS once, member-major with a row stride of
// ENS_LDR = 65 doubles (ds_read_b64 banks are (a / 4) mod 64, i.e. 32 doubles per bank row: the four row classes of eight consecutive
// member blocks land on 32 different doubles), then
//   * totals: thread m adds the chunk's rows of member m in ascending row order, t <- fma(a_n, x_n, t) (a absent: t <- t + x_n);
//   * squared distances: the nb (nb + 1) / 2 pairs of member blocks (bi <= bj, numbered bj (bj + 1) / 2 + bi) are dealt to groups of four
//     lanes; lane q of a group owns the row class q = the chunk's rows q, q + 4, q + 8, ... and a 4 x 4 register block of member pairs:
//     per row 8 LDS reads, 16 differences d = u - v and 16 times acc <- fma(a_n d, d, acc) (a absent: fma(d, d, acc)), rows ascending;
//     the four classes are then added as ((q0 + q1) + q2) + q3.  The difference is formed first: never a Gram form.
//   Chunk partials go to a device buffer: [chunk][block pair][4][4] and [chunk][P].
// k_ens_reduce: one thread per element adds the chunks of a group in ascending chunk order (from +0) and leaves the sum -- for a pair
//   its correctly rounded square root, D -- in the group's first chunk slot.
// k_ens_vario<PM>, one workgroup per 64 x 64 tile of row pairs of a group (tiles ti <= tj, numbered tj (tj + 1) / 2 + ti): a thread
//   owns 4 x 4 row pairs (rows i = 4 (t / 16) + k of tile ti, j = 4 (t mod 16) + l of tile tj) and walks s in ascending order,
//   m <- m + |E_si - E_sj|^p with p = 1/2: sqrt(fabs), p = 1: fabs, p = 2: fma(d, d, m) (no pow); then, k outer and l inner over its pairs
//   with i < j, w <- fma((a_i a_j) r, r, w), r = |y_i - y_j|^p - m / S; the workgroup's sum is block_sum (the xor tree of a wave, the four
//   waves in order).  The members are staged through LDS 32 at a time.
// k_ens_finish, one workgroup per group (all sums sequential, from +0):
//   * c_t = sum_{s<t} D(s, t), s ascending, for t = 1 .. S (c_S is the sum against the observation);
//     energy = c_S / S - (sum_{t=1}^{S-1} c_t, t ascending) / den,   den = S^2, or S (S - 1) when fair;
//   * crps_total the same with |T_s - T_t| in place of D(s, t);
//   * variogram = the group's tile partials in ascending tile order;  dist = D mirrored, zero diagonal.
// No atomics; each output element has ONE order, which depends on S and the group's own rows only.
// Resources on gfx950 (-Rpass-analysis=kernel-resource-usage) are listed in DESIGN.md 10f; no kernel uses scratch.
#include "zigp_rows.h"
#include <climits>
#include <cmath>

using namespace zigp;

namespace zigp {

constexpr int ENS_CH = ZIGP_ENS_CHUNK;        // rows of a chunk
constexpr int ENS_LDR = ENS_CH + 1;           // row stride of a member in LDS, doubles
constexpr int ENS_THREADS = 256;              // at most; k_ens_pairs runs 64 .. 256 by the number of block pairs
constexpr int ENS_MAX_S = ZIGP_PATH_MAX_S;
constexpr int ENS_MAX_NB = (ENS_MAX_S + 1 + 3) / 4;
constexpr size_t ENS_MAX_LDS = sizeof(double) * ((size_t)4 * ENS_MAX_NB * ENS_LDR + ENS_CH);   // 135 712 bytes of the CU's 160 KiB
constexpr int VG_T = 64;                      // rows of a variogram tile
constexpr int VG_SB = 32;                     // members staged at a time
constexpr int VG_THREADS = 256;
static_assert(ENS_CH == 64, "k_ens_pairs decodes a staged index with >> 6 and & 63");
static_assert(ZIGP_ENS_VARIO_MAX_ROWS % VG_T == 0, "whole tiles");

struct EnsArgs {
  const double* E; int64_t ld; int S;     // members [S] rows of stride ld
  const double* y; const double* a;       // [N]; a nullable
  const int* off;                         // [G + 1] row boundaries
  const int* cstart;                      // [G + 1] chunk prefix counts
  const int* vstart;                      // [G + 1] variogram tile prefix counts
  int G, nb;                              // groups; member blocks of four
  double* ppair;                          // [chunks][nb (nb + 1) / 2][16] (nullable)
  double* ptot;                           // [chunks][S + 1] (nullable)
  double* pv;                             // [tiles] (nullable)
  double den;                             // S^2 or S (S - 1)
  double* total; double* total_obs; double* crps_total; double* energy; double* variogram; double* dist;   // outputs (nullable)
};

// The g with start[g] <= c < start[g + 1]; start[0] = 0 <= c < start[G]
__device__ __forceinline__ int ens_group_of(const int* __restrict__ start, int G, int c) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid + 1] <= c) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// e = j (j + 1) / 2 + i with i <= j
__device__ __forceinline__ void ens_tri(int e, int& i, int& j) {
  j = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (j * (j + 1) / 2 > e) --j;
  while ((j + 1) * (j + 2) / 2 <= e) ++j;
  i = e - j * (j + 1) / 2;
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(ENS_THREADS)
k_ens_pairs(EnsArgs p) {
  extern __shared__ double ens_sh[];
  const int c = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int g = ens_group_of(p.cstart, p.G, c);
  const int r0 = p.off[g] + (c - p.cstart[g]) * ENS_CH, nr = min(ENS_CH, p.off[g + 1] - r0);
  const int P = p.S + 1, PP = 4 * p.nb;
  double* tile = ens_sh;
  double* wt = ens_sh + PP * ENS_LDR;
  for (int idx = tid; idx < PP * ENS_CH; idx += nt) {
    const int m = idx >> 6, r = idx & 63;
    double v = 0.0;
    if (r < nr && m < P) v = m < p.S ? p.E[(int64_t)m * p.ld + r0 + r] : p.y[(int64_t)r0 + r];
    tile[m * ENS_LDR + r] = v;
  }
  if (tid < ENS_CH) wt[tid] = (WEIGHTED && tid < nr) ? p.a[(int64_t)r0 + tid] : 1.0;
  __syncthreads();
  if (p.ptot)
    for (int m = tid; m < P; m += nt) {
      const double* x = tile + m * ENS_LDR;
      double t = 0.0;
      for (int r = 0; r < nr; ++r) t = WEIGHTED ? fma(wt[r], x[r], t) : t + x[r];
      p.ptot[(int64_t)c * P + m] = t;
    }
  if (!p.ppair) return;
  const int q = tid & 3, per = nt >> 2, nblk = p.nb * (p.nb + 1) / 2, lane = tid & 63, base = lane & ~3;
  const int ni = nr > q ? (nr - q + 3) >> 2 : 0;
  for (int b0 = 0; b0 < nblk; b0 += per) {        // uniform over the workgroup: every lane takes part in the shuffles
    const int b = b0 + (tid >> 2);
    double acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = 0; l < 4; ++l) acc[k][l] = 0.0;
    if (b < nblk) {
      int bi, bj;
      ens_tri(b, bi, bj);
      const double* U = tile + 4 * bi * ENS_LDR + q;
      const double* V = tile + 4 * bj * ENS_LDR + q;
      for (int i = 0; i < ni; ++i) {
        const int r = 4 * i;
        const double w = wt[r + q];
        double u[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { u[k] = U[k * ENS_LDR + r]; v[k] = V[k * ENS_LDR + r]; }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            const double d = u[k] - v[l];
            acc[k][l] = WEIGHTED ? fma(w * d, d, acc[k][l]) : fma(d, d, acc[k][l]);
          }
      }
    }
    double mine[4] = {0.0, 0.0, 0.0, 0.0};      // lane q of the four keeps row k = q of the block
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const double x = acc[k][l];
        const double s = ((__shfl(x, base, 64) + __shfl(x, base + 1, 64)) + __shfl(x, base + 2, 64)) + __shfl(x, base + 3, 64);
        if (k == q) mine[l] = s;
      }
    if (b < nblk) {
      double* o = p.ppair + ((int64_t)c * nblk + b) * 16 + q * 4;
#pragma unroll
      for (int l = 0; l < 4; ++l) o[l] = mine[l];
    }
  }
}

// Elements of a group: its pair sums (-> D) where they are asked for, then its P totals.  Work item = (group, block of 256 elements).
__global__ void __launch_bounds__(256)
k_ens_reduce(EnsArgs p, int npe, int nbx) {
  const int P = p.S + 1, np = p.ppair ? npe : 0, ne = np + (p.ptot ? P : 0);
  const int64_t W = (int64_t)p.G * nbx;
  for (int64_t w = blockIdx.x; w < W; w += gridDim.x) {
    const int g = (int)(w / nbx), e = (int)(w - (int64_t)g * nbx) * 256 + threadIdx.x;
    const int c0 = p.cstart[g], c1 = p.cstart[g + 1];
    if (e >= ne || c1 == c0) continue;
    double v = 0.0;
    if (e < np) {
      for (int c = c0; c < c1; ++c) v += p.ppair[(int64_t)c * npe + e];
      p.ppair[(int64_t)c0 * npe + e] = sqrt(v);
    } else {
      const int m = e - np;
      for (int c = c0; c < c1; ++c) v += p.ptot[(int64_t)c * P + m];
      p.ptot[(int64_t)c0 * P + m] = v;
    }
  }
}

template <int PM> __device__ __forceinline__ double ens_pow_add(double d, double acc) {   // acc + |d|^p; PM = 0: p = 1/2, 1: p = 1, 2: p = 2
  if constexpr (PM == 0) return acc + sqrt(fabs(d));
  else if constexpr (PM == 1) return acc + fabs(d);
  else return fma(d, d, acc);
}

template <int PM>
__global__ void __launch_bounds__(VG_THREADS)
k_ens_vario(EnsArgs p) {
  __shared__ double A[VG_SB][VG_T], B[VG_SB][VG_T];
  __shared__ double sh[VG_THREADS / 64];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int g = ens_group_of(p.vstart, p.G, w);
  int ti, tj;
  ens_tri(w - p.vstart[g], ti, tj);
  const int n = p.off[g + 1] - p.off[g];
  const int64_t i0 = (int64_t)p.off[g] + ti * VG_T, j0 = (int64_t)p.off[g] + tj * VG_T;
  const int ni = min(VG_T, n - ti * VG_T), nj = min(VG_T, n - tj * VG_T);
  const int ii = (tid >> 4) * 4, jj = (tid & 15) * 4;
  double acc[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int l = 0; l < 4; ++l) acc[k][l] = 0.0;
  for (int s0 = 0; s0 < p.S; s0 += VG_SB) {
    const int sb = min(VG_SB, p.S - s0);
    __syncthreads();
    for (int idx = tid; idx < VG_SB * VG_T; idx += VG_THREADS) {
      const int m = idx >> 6, r = idx & 63;
      const double* row = p.E + (int64_t)(s0 + m) * p.ld;
      A[m][r] = (m < sb && r < ni) ? row[i0 + r] : 0.0;
      B[m][r] = (m < sb && r < nj) ? row[j0 + r] : 0.0;
    }
    __syncthreads();
    for (int m = 0; m < sb; ++m) {
      double u[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { u[k] = A[m][ii + k]; v[k] = B[m][jj + k]; }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[k][l] = ens_pow_add<PM>(u[k] - v[l], acc[k][l]);
    }
  }
  const double Sd = (double)p.S;
  double ws = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int li = ii + k, lj = jj + l;
      if (li < ni && lj < nj && ti * VG_T + li < tj * VG_T + lj) {
        const double ob = ens_pow_add<PM>(p.y[i0 + li] - p.y[j0 + lj], 0.0);
        const double r = ob - acc[k][l] / Sd;
        const double aa = p.a ? p.a[i0 + li] * p.a[j0 + lj] : 1.0;
        ws = fma(aa * r, r, ws);
      }
    }
  const double tot = block_sum<VG_THREADS / 64>(ws, sh);
  if (tid == 0) p.pv[w] = tot;
}

// D(u, v), u < v, of a group whose reduced pair block starts at `base`
__device__ __forceinline__ double ens_D(const double* __restrict__ base, int u, int v) {
  const int bi = u >> 2, bj = v >> 2;
  return base[(bj * (bj + 1) / 2 + bi) * 16 + (u & 3) * 4 + (v & 3)];
}

__global__ void __launch_bounds__(256)
k_ens_finish(EnsArgs p) {
  __shared__ double T[ENS_MAX_S + 1], cs[ENS_MAX_S + 1];
  const int g = blockIdx.x, tid = threadIdx.x, S = p.S, P = S + 1;
  const int c0 = p.cstart[g];
  const bool some = p.cstart[g + 1] > c0;      // an empty group has no chunk: all its outputs are +0
  const double Sd = (double)S;
  if (p.ptot) {
    for (int m = tid; m < P; m += 256) T[m] = some ? p.ptot[(int64_t)c0 * P + m] : 0.0;
    __syncthreads();
    if (p.total)
      for (int s = tid; s < S; s += 256) p.total[(int64_t)s * p.G + g] = T[s];
    if (p.total_obs && tid == 0) p.total_obs[g] = T[S];
    if (p.crps_total) {
      for (int t = tid; t < P; t += 256) {
        double c = 0.0;
        for (int s = 0; s < t; ++s) c += fabs(T[s] - T[t]);
        cs[t] = c;
      }
      __syncthreads();
      if (tid == 0) {
        double s2 = 0.0;
        for (int t = 1; t < S; ++t) s2 += cs[t];
        p.crps_total[g] = __dsub_rn(__ddiv_rn(cs[S], Sd), __ddiv_rn(s2, p.den));
      }
      __syncthreads();
    }
  }
  if (p.ppair) {
    const int npe = p.nb * (p.nb + 1) / 2 * 16;
    const double* base = p.ppair + (int64_t)c0 * npe;
    if (p.energy) {
      for (int t = tid; t < P; t += 256) {
        double c = 0.0;
        if (some)
          for (int s = 0; s < t; ++s) c += ens_D(base, s, t);
        cs[t] = c;
      }
      __syncthreads();
      if (tid == 0) {
        double s2 = 0.0;
        for (int t = 1; t < S; ++t) s2 += cs[t];
        p.energy[g] = __dsub_rn(__ddiv_rn(cs[S], Sd), __ddiv_rn(s2, p.den));
      }
    }
    if (p.dist) {
      double* o = p.dist + (int64_t)g * P * P;
      for (int idx = tid; idx < P * P; idx += 256) {
        const int u = idx / P, v = idx - u * P;
        o[idx] = (u == v || !some) ? 0.0 : ens_D(base, min(u, v), max(u, v));
      }
    }
  }
  if (p.variogram && tid == 64) {
    double v = 0.0;
    for (int w = p.vstart[g]; w < p.vstart[g + 1]; ++w) v += p.pv[w];
    p.variogram[g] = v;
  }
}

}  // namespace zigp

namespace {

// The two zigp_ensemble_scores* entries.  on_device: E, y, a and the outputs are device memory, read and written in place; else they
// are the host's: E, y and a are staged into c->scratch as [E (S, N) | y | a], the outputs into slots of c->scratch2.  The regions of
// c->scratch2, in allocation order: the three index arrays (int32: row boundaries, chunk and tile prefix counts), the pair partials,
// the total partials, the tile partials, then the output slots.
int ensemble_scores(zigp_ctx* c, const char* who, bool on_device, const double* E, int64_t ld, int S, int64_t N, const double* y, const double* a,
                    const int64_t* off, int G, const zigp_ens_opts* opts, double* total, double* total_obs, double* crps_total, double* energy,
                    double* variogram, double* dist) {
  if (!c) return ZIGP_EARG;
  if (S < 1 || S > ENS_MAX_S) return refuse(c, who, "S must be in [1, 256] (ZIGP_PATH_MAX_S)");
  if (N < 1 || N > (int64_t)INT_MAX) return refuse(c, who, "N must be in [1, 2^31)");
  if (ld < N) return refuse(c, who, "ld must be at least N");
  if (!E || !y) return refuse(c, who, "E or y is NULL");
  if (G < 1 || !off) return refuse(c, who, "G must be at least 1 and off must hold G + 1 boundaries");
  if (off[0] != 0 || off[G] != N) return refuse(c, who, "off must start at 0 and end at N");
  for (int g = 0; g < G; ++g)
    if (off[g + 1] < off[g]) return refuse(c, who, "off must be non-decreasing");
  const int fair = opts ? opts->fair : 0;
  const double vp = opts ? opts->vario_p : 0.0;
  if (fair != 0 && fair != 1) return refuse(c, who, "fair must be 0 or 1");
  if (fair == 1 && S == 1) return refuse(c, who, "fair = 1 needs S >= 2 (c = 1 / (S (S - 1)))");
  if (!(vp == 0.0 || vp == 0.5 || vp == 1.0 || vp == 2.0)) return refuse(c, who, "vario_p must be 0.5, 1 or 2 (0: no variogram)");
  if ((variogram != nullptr) != (vp != 0.0)) return refuse(c, who, "vario_p and variogram go together: vario_p = 0 with variogram NULL, or both set");
  if (variogram)
    for (int g = 0; g < G; ++g)
      if (off[g + 1] - off[g] > ZIGP_ENS_VARIO_MAX_ROWS)
        return refuse(c, who, "variogram: a group of off has more than 4096 rows (ZIGP_ENS_VARIO_MAX_ROWS)");
  if (!on_device && a)
    for (int64_t n = 0; n < N; ++n)
      if (!(a[n] >= 0.0) || !std::isfinite(a[n])) return refuse(c, who, "a (the row weights) must be finite and >= 0");
  const bool want_pairs = energy || dist, want_tot = total || total_obs || crps_total;
  if (!want_pairs && !want_tot && !variogram) return ZIGP_OK;
  ZIGP_HIP(c, hipSetDevice(c->device));
  if (on_device)
    ZIGP_TRY(require_device_ptrs(c, {E, y, a, total, total_obs, crps_total, energy, variogram, dist},
                                 (std::string(who) + ": E, y, a and the outputs must be device memory of the context's GPU").c_str()));
  ZIGP_TRY(begin_staged_call(c));
  // the index arrays, through the pinned arena
  const size_t ni = (size_t)G + 1;
  int* h_idx = (int*)c->pinned.alloc(sizeof(int) * 3 * ni);
  if (!h_idx) { c->err = "hipHostMalloc failed for the staging arena"; return ZIGP_EHIP; }
  int* h_off = h_idx; int* h_cs = h_idx + ni; int* h_vs = h_idx + 2 * ni;
  int64_t nc = 0, nv = 0;
  for (int g = 0; g <= G; ++g) {
    h_off[g] = (int)off[g]; h_cs[g] = (int)nc; h_vs[g] = (int)nv;
    if (g == G) break;
    const int64_t n = off[g + 1] - off[g];
    nc += (n + ENS_CH - 1) / ENS_CH;
    if (variogram) { const int64_t t = (n + VG_T - 1) / VG_T; nv += t * (t + 1) / 2; }
    if (nv > (int64_t)INT_MAX) return refuse(c, who, "variogram: more than 2^31 tiles of row pairs");
  }
  const int P = S + 1, nb = (P + 3) / 4, nblk = nb * (nb + 1) / 2, npe = nblk * 16;

  if (!on_device) {
    RowArena in(c->scratch, "c->scratch");
    const size_t oe = in.take((size_t)S * N), oy = in.take(N), oa = in.take(a ? (size_t)N : 0);
    ZIGP_TRY(in.commit(c));
    ZIGP_HIP(c, hipMemcpy2DAsync(in.at(oe), sizeof(double) * N, E, sizeof(double) * ld, sizeof(double) * N, S, hipMemcpyHostToDevice, c->stream));
    ZIGP_HIP(c, hipMemcpyAsync(in.at(oy), y, sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    if (a) ZIGP_HIP(c, hipMemcpyAsync(in.at(oa), a, sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    E = in.at(oe); ld = N; y = in.at(oy);
    if (a) a = in.at(oa);
  }
  RowArena ar(c->scratch2, "c->scratch2");
  const size_t o_idx = ar.take((3 * ni + 1) / 2);
  const size_t o_pair = ar.take(want_pairs ? (size_t)nc * npe : 0), o_tot = ar.take(want_tot ? (size_t)nc * P : 0), o_pv = ar.take((size_t)nv);
  const size_t o_total = ar.take(total ? (size_t)S * G : 0), o_tobs = ar.take(total_obs ? G : 0), o_crps = ar.take(crps_total ? G : 0);
  const size_t o_en = ar.take(energy ? G : 0), o_vg = ar.take(variogram ? G : 0), o_dist = ar.take(dist ? (size_t)G * P * P : 0);
  ZIGP_TRY(ar.commit(c));
  int* d_idx = (int*)ar.at(o_idx);
  ZIGP_HIP(c, hipMemcpyAsync(d_idx, h_idx, sizeof(int) * 3 * ni, hipMemcpyHostToDevice, c->stream));

  EnsArgs p{};
  p.E = E; p.ld = ld; p.S = S; p.y = y; p.a = a;
  p.off = d_idx; p.cstart = d_idx + ni; p.vstart = d_idx + 2 * ni; p.G = G; p.nb = nb;
  p.ppair = want_pairs ? ar.at(o_pair) : nullptr; p.ptot = want_tot ? ar.at(o_tot) : nullptr; p.pv = variogram ? ar.at(o_pv) : nullptr;
  p.den = fair ? (double)S * (double)(S - 1) : (double)S * (double)S;
  p.total = out_target(total, on_device, ar.at(o_total)); p.total_obs = out_target(total_obs, on_device, ar.at(o_tobs));
  p.crps_total = out_target(crps_total, on_device, ar.at(o_crps)); p.energy = out_target(energy, on_device, ar.at(o_en));
  p.variogram = out_target(variogram, on_device, ar.at(o_vg)); p.dist = out_target(dist, on_device, ar.at(o_dist));

  if (want_pairs || want_tot) {
    static bool attr_set = false;
    if (!attr_set) {
      ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ens_pairs<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ENS_MAX_LDS));
      ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ens_pairs<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ENS_MAX_LDS));
      attr_set = true;
    }
    const size_t shm = sizeof(double) * ((size_t)4 * nb * ENS_LDR + ENS_CH);
    const int threads = want_pairs ? (int)std::min<int64_t>(ENS_THREADS, round_up(4 * (int64_t)nblk, 64)) : (int)std::min<int64_t>(ENS_THREADS, round_up(P, 64));
    if (a) hipLaunchKernelGGL(k_ens_pairs<true>, dim3((unsigned)nc), dim3(threads), shm, c->stream, p);
    else hipLaunchKernelGGL(k_ens_pairs<false>, dim3((unsigned)nc), dim3(threads), shm, c->stream, p);
    ZIGP_HIP(c, hipGetLastError());
    const int nbx = ceil_div((want_pairs ? npe : 0) + (want_tot ? P : 0), 256);
    const int64_t W = (int64_t)G * nbx;
    hipLaunchKernelGGL(k_ens_reduce, dim3((unsigned)std::min<int64_t>(W, (int64_t)1 << 20)), dim3(256), 0, c->stream, p, npe, nbx);
    ZIGP_HIP(c, hipGetLastError());
  }
  if (variogram && nv > 0) {
    const dim3 grid((unsigned)nv), block(VG_THREADS);
    if (vp == 0.5) hipLaunchKernelGGL(k_ens_vario<0>, grid, block, 0, c->stream, p);
    else if (vp == 1.0) hipLaunchKernelGGL(k_ens_vario<1>, grid, block, 0, c->stream, p);
    else hipLaunchKernelGGL(k_ens_vario<2>, grid, block, 0, c->stream, p);
    ZIGP_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_ens_finish, dim3((unsigned)G), dim3(256), 0, c->stream, p);
  ZIGP_HIP(c, hipGetLastError());
  const bool h = !on_device;
  return finish_copies(c, {{h ? total : nullptr, ar.at(o_total), (size_t)S * G}, {h ? total_obs : nullptr, ar.at(o_tobs), (size_t)G},
                           {h ? crps_total : nullptr, ar.at(o_crps), (size_t)G}, {h ? energy : nullptr, ar.at(o_en), (size_t)G},
                           {h ? variogram : nullptr, ar.at(o_vg), (size_t)G}, {h ? dist : nullptr, ar.at(o_dist), (size_t)G * P * P}});
}

}  // namespace

extern "C" {

int zigp_ensemble_scores(zigp_ctx* c, const double* E, int64_t ld, int32_t S, int64_t N, const double* y, const double* a, const int64_t* off,
                         int32_t G, const zigp_ens_opts* opts, double* total, double* total_obs, double* crps_total, double* energy,
                         double* variogram, double* dist) {
  return ensemble_scores(c, "zigp_ensemble_scores", false, E, ld, S, N, y, a, off, G, opts, total, total_obs, crps_total, energy, variogram, dist);
}

int zigp_ensemble_scores_device(zigp_ctx* c, const double* dE, int64_t ld, int32_t S, int64_t N, const double* dy, const double* da,
                                const int64_t* off, int32_t G, const zigp_ens_opts* opts, double* d_total, double* d_total_obs,
                                double* d_crps_total, double* d_energy, double* d_variogram, double* d_dist) {
  return ensemble_scores(c, "zigp_ensemble_scores_device", true, dE, ld, S, N, dy, da, off, G, opts, d_total, d_total_obs, d_crps_total,
                         d_energy, d_variogram, d_dist);
}

}  // extern "C"
