// Inducing inputs by k-means on the device: Lloyd iterations (include/zigp.h "inducing inputs").
//
// THE definition (zigp.inducing.kmeans_np is its NumPy restatement).  X: N rows, the D columns from col0 of a row of stride ld; C (M, D).
// Iteration t = 1, 2, ... with the current C:
//   d(i, j)  = sum_k (x_ik - c_jk)^2, k ascending, the difference form (the first square rounded, every later one fused into the sum);
//   label_i  = the LOWEST j attaining min_j d(i, j);
//   c_j     <- sum_j / count_j over the rows of label j where count_j > 0; an empty cluster keeps its centroid;
//   inertia_t = sum_i d(i, label_i) against C before the update; changed_t = rows whose label differs from iteration t - 1, changed_1 = N.
// Stop after the first t with changed_t = 0, or at t = max_iter.
//
// k_kmeans_step<DT>: 256 threads; a workgroup owns a contiguous span of `tiles_per` tiles of 256 rows (the last span may be short).
// DT = 1..8: D = DT; a thread holds its row of each of KM_ROWS = 4 consecutive tiles of the span in registers and scores the four in
// one pass over the centroids, so a centroid is fetched once per four rows (the arithmetic of a row is that of one row per thread).
// DT = KM_WIDE (64): 9 <= D <= 64 at run time, one tile at a time: its rows sit in LDS ([k][256], conflict free) and four centroids
// are scored per pass over k, so a row element is read once per four centroids.  The centroid index is uniform over the workgroup and
// C is read-only in the launch: its loads are scalar loads through the constant cache and the fp64 VALU takes the values as scalar
// operands -- no LDS traffic in the D <= 8 inner loop, which is 2 D fp64 operations plus a compare and three selects per (row, centroid).
// Sums, fixed order and no atomics.  After a tile's labels are known every thread writes its label and its row to LDS; thread t OWNS the
// centroids t, t + 256, ... and walks the tile's 256 labels once, IN ROW ORDER, taking the rows of its own centroids.  The running sums
// and the count of the centroid it took last stay in registers; when the next row belongs to another of its centroids they go to the
// workgroup's partial block part[g][k][j] (k = D: the count, a double) and that centroid's are loaded -- so every partial is the plain
// left-to-right sum of its rows in row order, whatever the tile and the owner.  One label compare per row and thread, independent of M.
// k_kmeans_finish adds the G partials of an entry -- four quarters of the workgroups, each in ascending g, then the quarters in order --
// divides and writes C, the counts and the history row; the inertia is [per thread: its rows in tile order] -> [wave xor tree, then the
// four waves in order] -> [256 runs of consecutive workgroups, each in ascending g, then the same tree].
// G follows from (N, M, D) alone (km_plan), so the host, device-pointer and resident forms agree bit for bit.
// The loop has no host synchronisation per iteration: finish t writes flags[t] = (changed_t == 0 or flags[t - 1]) and every launch of
// iteration t + 1 returns at once when flags[t] is set (a launch reads flags[t - 1] and writes flags[t]: no launch reads what it writes).
// The host looks after iteration 1 (the non-finite refusal) and then every KM_LOOK iterations; n_iter is the first t with changed_t = 0
// however often it looks, and the update of that iteration reproduces C bit for bit.
// Resources on gfx950 (-Rpass-analysis=kernel-resource-usage): the table in DESIGN.md section 11; no scratch in any kernel.
#include "zigp_host.h"
#include <cmath>

using namespace zigp;

namespace zigp {

constexpr int KM_THREADS = 256;          // threads per workgroup = rows per tile
constexpr int KM_WIDE = 64;              // template argument of the run-time-D kernel (= ZIGP_MAX_D)
constexpr int KM_ROWS = 4;               // D <= 8: rows per thread and pass over the centroids (a row of each of 4 consecutive tiles of the span)
constexpr int KM_MAX_GROUPS = 1024;      // workgroups of a step at most: 4 per CU of a 256-CU chip
constexpr size_t KM_PART_BUDGET = (size_t)1 << 24;   // doubles of partial sums at most (128 MB): fewer workgroups at a large M (D + 1)
constexpr int KM_LOOK = 8;               // iterations enqueued between two looks at the device's flag
constexpr int KM_MAX_ITER = 1 << 20;
static_assert(KM_WIDE == ZIGP_MAX_D, "include/zigp.h");
#ifdef ZIGP_KMEANS_NO_SCAN               // the second arm of tools/kmeans_time.py: no owner scan, so no update and no stop -- timing only
constexpr bool KM_SCAN = false;
#else
constexpr bool KM_SCAN = true;
#endif

// The owner's registers <-> its entry of the workgroup's partial block.  k runs to the template bound with a uniform test against the
// run-time D, so the register array is indexed by constants only.
template <int DT>
__device__ __forceinline__ void km_load(const double* __restrict__ myp, int M, int D, int j, double (&acc)[DT], double& cnt) {
#pragma unroll
  for (int k = 0; k < DT; ++k)
    if (k < D) acc[k] = myp[(size_t)k * M + j];
  cnt = myp[(size_t)D * M + j];
}
template <int DT>
__device__ __forceinline__ void km_store(double* __restrict__ myp, int M, int D, int j, const double (&acc)[DT], double cnt) {
#pragma unroll
  for (int k = 0; k < DT; ++k)
    if (k < D) myp[(size_t)k * M + j] = acc[k];
  myp[(size_t)D * M + j] = cnt;
}

template <int DT>
__global__ void __launch_bounds__(KM_THREADS)
k_kmeans_step(const double* __restrict__ X, const double* __restrict__ C, int* __restrict__ labels, double* __restrict__ part,
              double* __restrict__ part_inertia, int* __restrict__ part_changed, const int* __restrict__ done_prev, int64_t N, int ld,
              int col0, int M, int Dw, int ntiles, int tiles_per, int first) {
  constexpr bool WIDE = DT == KM_WIDE;
  constexpr int R = WIDE ? 1 : KM_ROWS;
  const int D = WIDE ? Dw : DT;
  if (*done_prev) return;
  extern __shared__ double km_wide_rows[];                          // WIDE: [D][256]
  __shared__ double xs_narrow[WIDE ? 1 : DT * KM_THREADS];          // D <= 8: [D][256]
  __shared__ int ls[KM_THREADS];
  __shared__ double red[KM_THREADS / 64];
  __shared__ int redc[KM_THREADS / 64];
  double* xs = WIDE ? km_wide_rows : xs_narrow;
  const int t = threadIdx.x, g = blockIdx.x;
  double* myp = part + (size_t)g * (size_t)(D + 1) * M;
  for (int j = t; j < M; j += KM_THREADS)
    for (int k = 0; k <= D; ++k) myp[(size_t)k * M + j] = 0.0;
  double acc[DT], cnt = 0.0, inertia = 0.0;
#pragma unroll
  for (int k = 0; k < DT; ++k) acc[k] = 0.0;
  int cur = -1, changed = 0;
  const int tile_end = min(ntiles, (g + 1) * tiles_per);
  for (int tile0 = g * tiles_per; tile0 < tile_end; tile0 += R) {    // R tiles at a time: one pass over the centroids scores a row of each
    double best[R], x[R][WIDE ? 1 : DT];
    int lab[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r] = INFINITY; lab[r] = 0; }
    if constexpr (!WIDE) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t row = (int64_t)(tile0 + r) * KM_THREADS + t;
        const double* xr = X + ((tile0 + r < tile_end && row < N) ? row : 0) * (int64_t)ld + col0;
#pragma unroll
        for (int k = 0; k < DT; ++k) x[r][k] = xr[k];
      }
#pragma unroll 2
      for (int j = 0; j < M; ++j) {
        const double* cj = C + (size_t)j * DT;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          double e = x[r][0] - cj[0], d = e * e;
#pragma unroll
          for (int k = 1; k < DT; ++k) { e = x[r][k] - cj[k]; d = fma(e, e, d); }
          const bool lt = d < best[r];                                // strict: the lowest j wins a tie; false on NaN
          best[r] = lt ? d : best[r]; lab[r] = lt ? j : lab[r];
        }
      }
    } else {
      const int64_t row = (int64_t)tile0 * KM_THREADS + t;
      const double* xr = X + (row < N ? row : 0) * (int64_t)ld + col0;
      for (int k = 0; k < D; ++k) xs[k * KM_THREADS + t] = xr[k];     // own column of the tile: read back by this thread only, until the scan
      for (int j0 = 0; j0 < M; j0 += 4) {
        const double* c0 = C + (size_t)j0 * D;
        const double* c1 = C + (size_t)min(j0 + 1, M - 1) * D;
        const double* c2 = C + (size_t)min(j0 + 2, M - 1) * D;
        const double* c3 = C + (size_t)min(j0 + 3, M - 1) * D;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;                // fma(e, e, 0) = the rounded square: the D <= 8 kernels' bits
        for (int k = 0; k < D; ++k) {
          const double xv = xs[k * KM_THREADS + t];
          const double e0 = xv - c0[k], e1 = xv - c1[k], e2 = xv - c2[k], e3 = xv - c3[k];
          d0 = fma(e0, e0, d0); d1 = fma(e1, e1, d1); d2 = fma(e2, e2, d2); d3 = fma(e3, e3, d3);
        }
        bool lt = d0 < best[0];
        best[0] = lt ? d0 : best[0]; lab[0] = lt ? j0 : lab[0];
        lt = j0 + 1 < M && d1 < best[0]; best[0] = lt ? d1 : best[0]; lab[0] = lt ? j0 + 1 : lab[0];
        lt = j0 + 2 < M && d2 < best[0]; best[0] = lt ? d2 : best[0]; lab[0] = lt ? j0 + 2 : lab[0];
        lt = j0 + 3 < M && d3 < best[0]; best[0] = lt ? d3 : best[0]; lab[0] = lt ? j0 + 3 : lab[0];
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {                                     // the tiles of the group one after the other, in row order
      if (tile0 + r >= tile_end) break;
      const int64_t row = (int64_t)(tile0 + r) * KM_THREADS + t;
      const bool valid = row < N;
      if (valid) {
        changed += (first || labels[row] != lab[r]) ? 1 : 0;
        labels[row] = lab[r];
        inertia += best[r];
      }
      ls[t] = valid ? lab[r] : -1;
      if constexpr (!WIDE) {
#pragma unroll
        for (int k = 0; k < DT; ++k) xs[k * KM_THREADS + t] = x[r][k];
      }
      __syncthreads();
      for (int i = 0; KM_SCAN && i < KM_THREADS; ++i) {
        const int l = ls[i];
        if (l >= 0 && (l & (KM_THREADS - 1)) == t) {                  // a row of one of this thread's centroids
          if (l != cur) {
            if (cur >= 0) km_store<DT>(myp, M, D, cur, acc, cnt);
            km_load<DT>(myp, M, D, l, acc, cnt);
            cur = l;
          }
#pragma unroll
          for (int k = 0; k < DT; ++k)
            if (k < D) acc[k] += xs[k * KM_THREADS + i];
          cnt += 1.0;
        }
      }
      __syncthreads();
    }
  }
  if (cur >= 0) km_store<DT>(myp, M, D, cur, acc, cnt);
  const double s = block_sum<KM_THREADS / 64>(inertia, red);
  int ch = changed;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ch += __shfl_xor(ch, o, 64);
  if ((t & 63) == 0) redc[t >> 6] = ch;
  __syncthreads();
  if (t == 0) {
    part_inertia[g] = s;
    part_changed[g] = (redc[0] + redc[1]) + (redc[2] + redc[3]);
  }
}

// Grid (ceil(M / 64), D + 2), 256 threads.  Row y <= D of the grid: wave q of a block adds the q-th quarter of the G partials of entry
// (y, j) for 64 consecutive centroids j, in ascending g (eight loads in flight, the adds in order), and wave 0 adds the four quarters in
// order -- y < D: the sum and the count, the division, C; y = D: the count alone, counts.  A serial walk over all G by one thread per
// centroid is a chain of G (D + 1) load latencies: 1.2 ms at the cfg3 shape, more than the step kernel.  Row y = D + 1, block 0: the
// inertia (a thread adds a contiguous run of workgroups in ascending g, then the block's tree) and changed, the history row, the flag.
__global__ void __launch_bounds__(KM_THREADS)
k_kmeans_finish(const double* __restrict__ part, const double* __restrict__ part_inertia, const int* __restrict__ part_changed, int G, int M,
                int D, double* __restrict__ C, int64_t* __restrict__ counts, double* __restrict__ hist, int* __restrict__ flags, int t) {
  const int y = blockIdx.y, tid = threadIdx.x;
  const bool tail_block = y == D + 1 && blockIdx.x == 0;
  if (flags[t - 1]) {
    if (tail_block && tid == 0) flags[t] = 1;
    return;
  }
  __shared__ double sh[2][KM_THREADS / 64][64];
  __shared__ double red[KM_THREADS / 64];
  __shared__ long long redc[KM_THREADS / 64];
  if (y == D + 1) {
    if (!tail_block) return;
    const int per = (G + KM_THREADS - 1) / KM_THREADS;
    double inertia = 0.0;
    long long ch = 0;
    for (int g = tid * per; g < min(G, (tid + 1) * per); ++g) { inertia += part_inertia[g]; ch += part_changed[g]; }
    inertia = block_sum<KM_THREADS / 64>(inertia, red);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ch += __shfl_xor(ch, o, 64);
    if ((tid & 63) == 0) redc[tid >> 6] = ch;
    __syncthreads();
    if (tid == 0) {
      ch = (redc[0] + redc[1]) + (redc[2] + redc[3]);
      hist[2 * (t - 1)] = inertia; hist[2 * (t - 1) + 1] = (double)ch;
      flags[t] = (KM_SCAN && ch == 0) ? 1 : 0;
    }
    return;
  }
  const int q = tid >> 6, lane = tid & 63, j = blockIdx.x * 64 + lane;
  const int gper = (G + 3) / 4, g0 = q * gper, g1 = min(G, g0 + gper);
  const size_t slab = (size_t)(D + 1) * M;
  double cnt = 0.0, s = 0.0;
  if (j < M) {
#pragma unroll 8
    for (int g = g0; g < g1; ++g) cnt += part[g * slab + (size_t)D * M + j];
    if (y < D) {
#pragma unroll 8
      for (int g = g0; g < g1; ++g) s += part[g * slab + (size_t)y * M + j];
    }
  }
  sh[0][q][lane] = cnt; sh[1][q][lane] = s;
  __syncthreads();
  if (q == 0 && j < M) {
    cnt = ((sh[0][0][lane] + sh[0][1][lane]) + sh[0][2][lane]) + sh[0][3][lane];
    s = ((sh[1][0][lane] + sh[1][1][lane]) + sh[1][2][lane]) + sh[1][3][lane];
    if (y == D) counts[j] = (int64_t)cnt;
    else if (cnt > 0.0) C[(size_t)j * D + y] = s / cnt;
  }
}

}  // namespace zigp

namespace {

// Workgroups of a step and tiles per workgroup: a function of (N, M, D) alone
struct KmPlan { int ntiles, tiles_per, G; };
KmPlan km_plan(int64_t N, int M, int D) {
  KmPlan p;
  p.ntiles = ceil_div(N, KM_THREADS);
  const size_t per = (size_t)M * (D + 1);
  const int cap = (int)std::max<size_t>(1, std::min<size_t>(KM_MAX_GROUPS, KM_PART_BUDGET / per));
  p.tiles_per = ceil_div(p.ntiles, std::min(p.ntiles, cap));
  if (D <= 8 && p.tiles_per < KM_ROWS && p.ntiles >= KM_ROWS * 512) p.tiles_per = KM_ROWS;   // whole groups of KM_ROWS tiles while 512 workgroups remain
  p.G = ceil_div(p.ntiles, p.tiles_per);
  return p;
}

int km_launch_step(zigp_ctx* c, int D, const KmPlan& pl, const double* X, const double* C, int* labels, double* part, double* pi, int* pc,
                   const int* done_prev, int64_t N, int ld, int col0, int M, int first) {
  const dim3 grid(pl.G), block(KM_THREADS);
#define KM_STEP(DT, SHM) \
  hipLaunchKernelGGL((k_kmeans_step<DT>), grid, block, SHM, c->stream, X, C, labels, part, pi, pc, done_prev, N, ld, col0, M, D, pl.ntiles, pl.tiles_per, first)
  switch (D) {
    case 1: KM_STEP(1, 0); break;
    case 2: KM_STEP(2, 0); break;
    case 3: KM_STEP(3, 0); break;
    case 4: KM_STEP(4, 0); break;
    case 5: KM_STEP(5, 0); break;
    case 6: KM_STEP(6, 0); break;
    case 7: KM_STEP(7, 0); break;
    case 8: KM_STEP(8, 0); break;
    default: {
      const size_t shm = sizeof(double) * (size_t)D * KM_THREADS;     // at most 128 KB of the CU's 160
      static bool attr_set = false;
      if (!attr_set) {
        ZIGP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmeans_step<KM_WIDE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(sizeof(double) * KM_WIDE * KM_THREADS)));
        attr_set = true;
      }
      KM_STEP(KM_WIDE, shm);
    }
  }
#undef KM_STEP
  ZIGP_HIP(c, hipGetLastError());
  return 0;
}

// Everything a k-means call refuses before it touches the device
int km_check(zigp_ctx* c, const char* who, int64_t N, int ld, int col0, int D, int M, const double* C, int max_iter, const int32_t* n_iter) {
  const std::string w(who);
  if (D < 1 || D > ZIGP_MAX_D) return fail_arg(c, (w + ": D must be in [1, 64] (ZIGP_MAX_D)").c_str());
  if (N < 1 || N >= ((int64_t)1 << 31)) return fail_arg(c, (w + ": N must be in [1, 2^31)").c_str());
  if (col0 < 0 || (int64_t)col0 + D > ld) return fail_arg(c, (w + ": col0 must be >= 0 and col0 + D <= ld (the row stride)").c_str());
  if (M < 1) return fail_arg(c, (w + ": M must be >= 1").c_str());
  if (M > ZIGP_KMEANS_MAX_M) return fail_arg(c, (w + ": M must be <= 4096 (ZIGP_KMEANS_MAX_M)").c_str());
  if (M > N) return fail_arg(c, (w + ": M must be <= N, the number of rows").c_str());
  if (max_iter < 1 || max_iter > KM_MAX_ITER) return fail_arg(c, (w + ": max_iter must be in [1, 1048576]").c_str());
  if (!C) return fail_arg(c, (w + ": C is NULL").c_str());
  if (!n_iter) return fail_arg(c, (w + ": n_iter is NULL").c_str());
  for (size_t i = 0; i < (size_t)M * D; ++i)     // a NaN centroid never wins a row, so the inertia would not show it
    if (!std::isfinite(C[i])) return fail_arg(c, (w + ": C is not finite: it holds a NaN or an infinity").c_str());
  return 0;
}

// The Lloyd loop over rows in device memory.  Every buffer of the call is owned by this scope and freed on every way out.
int km_run(zigp_ctx* c, const char* who, const double* dX, int64_t N, int ld, int col0, int D, int M, double* C, int max_iter,
           int32_t* labels, int64_t* counts, double* history, int32_t* n_iter) {
  const KmPlan pl = km_plan(N, M, D);
  DevBuf dC, part, pin, pch, lab, cnt, hist, flg;
  ZIGP_ENSURE(c, dC, (size_t)M * D);
  ZIGP_ENSURE(c, part, (size_t)pl.G * (D + 1) * M);
  ZIGP_ENSURE(c, pin, (size_t)pl.G);
  ZIGP_ENSURE(c, pch, (size_t)pl.G / 2 + 1);
  ZIGP_ENSURE(c, lab, (size_t)N / 2 + 1);
  ZIGP_ENSURE(c, cnt, (size_t)M);
  ZIGP_ENSURE(c, hist, (size_t)2 * max_iter);
  ZIGP_ENSURE(c, flg, (size_t)max_iter / 2 + 1);
  int* d_lab = reinterpret_cast<int*>(lab.p);
  int* d_pch = reinterpret_cast<int*>(pch.p);
  int* d_flg = reinterpret_cast<int*>(flg.p);                         // [max_iter + 1]
  int64_t* d_cnt = reinterpret_cast<int64_t*>(cnt.p);
  {
    ZIGP_PINNED(c, h, (size_t)M * D);
    memcpy(h, C, sizeof(double) * M * D);
    ZIGP_HIP(c, hipMemcpyAsync(dC.p, h, sizeof(double) * M * D, hipMemcpyHostToDevice, c->stream));
  }
  ZIGP_HIP(c, hipMemsetAsync(d_flg, 0, sizeof(int) * ((size_t)max_iter + 1), c->stream));
  ZIGP_PINNED(c, hflag, 1);                                           // an int32 in a slot of the arena
  int* hdone = reinterpret_cast<int*>(hflag);
  ZIGP_PINNED(c, hhist, (size_t)2 * max_iter);
  int t = 0;
  while (t < max_iter) {
    const int upto = t == 0 ? 1 : std::min(max_iter, t + KM_LOOK);
    for (; t < upto; ++t) {                                           // iteration t + 1
      ZIGP_TRY(km_launch_step(c, D, pl, dX, dC.p, d_lab, part.p, pin.p, d_pch, d_flg + t, N, ld, col0, M, t == 0 ? 1 : 0));
      hipLaunchKernelGGL(k_kmeans_finish, dim3(ceil_div(M, 64), D + 2), dim3(KM_THREADS), 0, c->stream, part.p, pin.p, d_pch, pl.G, M, D, dC.p,
                         d_cnt, hist.p, d_flg, t + 1);
      ZIGP_HIP(c, hipGetLastError());
    }
    ZIGP_HIP(c, hipMemcpyAsync(hdone, d_flg + t, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (t == 1) ZIGP_HIP(c, hipMemcpyAsync(hhist, hist.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ZIGP_HIP(c, hipStreamSynchronize(c->stream));
    if (t == 1 && !std::isfinite(hhist[0]))
      return fail_arg(c, (std::string(who) + ": the inertia of iteration 1 is not finite: X or C holds a non-finite value").c_str());
    if (*hdone) break;
  }
  // the iterations that ran: rows [0, t) of the device history up to and including the first with changed = 0
  ZIGP_HIP(c, hipMemcpyAsync(hhist, hist.p, sizeof(double) * 2 * t, hipMemcpyDeviceToHost, c->stream));
  double* hC = nullptr;
  ZIGP_TRY(download(c, dC.p, (size_t)M * D, &hC));
  if (labels) ZIGP_HIP(c, hipMemcpyAsync(labels, d_lab, sizeof(int32_t) * N, hipMemcpyDeviceToHost, c->stream));
  if (counts) ZIGP_HIP(c, hipMemcpyAsync(counts, d_cnt, sizeof(int64_t) * M, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  int n = t;
  for (int i = 0; i < t; ++i)
    if (hhist[2 * i + 1] == 0.0) { n = i + 1; break; }
  memcpy(C, hC, sizeof(double) * M * D);
  if (history) memcpy(history, hhist, sizeof(double) * 2 * n);
  *n_iter = n;
  return ZIGP_OK;
}

int km_entry(zigp_ctx* c, const char* who, const double* X, bool on_device, int64_t N, int ld, int col0, int D, int M, double* C, int max_iter,
             int32_t* labels, int64_t* counts, double* history, int32_t* n_iter) {
  if (!c) return ZIGP_EARG;
  ZIGP_TRY(km_check(c, who, N, ld, col0, D, M, C, max_iter, n_iter));
  if (!X) return fail_arg(c, (std::string(who) + ": X is NULL").c_str());
  ZIGP_HIP(c, hipSetDevice(c->device));
  ZIGP_TRY(begin_staged_call(c));
  if (on_device) {
    ZIGP_TRY(require_device_ptrs(c, {X}, (std::string(who) + ": dX must be device memory of the context's GPU").c_str()));
    return km_run(c, who, X, N, ld, col0, D, M, C, max_iter, labels, counts, history, n_iter);
  }
  DevBuf dX;
  ZIGP_ENSURE(c, dX, (size_t)N * ld);
  ZIGP_HIP(c, hipMemcpyAsync(dX.p, X, sizeof(double) * N * ld, hipMemcpyHostToDevice, c->stream));
  return km_run(c, who, dX.p, N, ld, col0, D, M, C, max_iter, labels, counts, history, n_iter);
}

}  // namespace

extern "C" {

int zigp_kmeans(zigp_ctx* c, const double* X, int64_t N, int32_t ld, int32_t col0, int32_t D, int32_t M, double* C, int32_t max_iter,
                int32_t* labels, int64_t* counts, double* history, int32_t* n_iter) {
  return km_entry(c, "zigp_kmeans", X, false, N, ld, col0, D, M, C, max_iter, labels, counts, history, n_iter);
}

int zigp_kmeans_device(zigp_ctx* c, const double* dX, int64_t N, int32_t ld, int32_t col0, int32_t D, int32_t M, double* C, int32_t max_iter,
                       int32_t* labels, int64_t* counts, double* history, int32_t* n_iter) {
  return km_entry(c, "zigp_kmeans_device", dX, true, N, ld, col0, D, M, C, max_iter, labels, counts, history, n_iter);
}

int zigp_kmeans_resident(zigp_ctx* c, int32_t col0, int32_t D, int32_t M, double* C, int32_t max_iter, int32_t* labels, int64_t* counts,
                         double* history, int32_t* n_iter) {
  if (!c) return ZIGP_EARG;
  if (!c->fullX) return fail_arg(c, "zigp_kmeans_resident: no resident data (call zigp_set_data or zigp_set_data_device first)");
  return km_entry(c, "zigp_kmeans_resident", c->fullX, true, c->fullN, c->D, col0, D, M, C, max_iter, labels, counts, history, n_iter);
}

}  // extern "C"
