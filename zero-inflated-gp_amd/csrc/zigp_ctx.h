// Context, error handling, device-buffer and profiling helpers shared by the dense and Kronecker paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include "../../include/zigp.h"
#include "../../include/zigp_diag.h"
#include "zigp_gemm.h"

namespace zigp {

struct DevBuf {
  double* p = nullptr;
  size_t cap = 0;  // doubles
  bool owned = true;   // false: p points into another buffer (alias)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), owned(o.owned) { o.p = nullptr; o.cap = 0; o.owned = true; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; owned = o.owned; o.p = nullptr; o.cap = 0; o.owned = true; }
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t n) {
    if (!owned) { p = nullptr; cap = 0; owned = true; }
    if (n <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    hipError_t e = hipMalloc((void**)&p, n * sizeof(double));
    if (e != hipSuccess) return -1;
    cap = n;
    return 0;
  }
  void alias(double* q, size_t n) { release(); p = q; cap = n; owned = false; }   // a view of n doubles at q (owned by someone else)
  void release() { if (p && owned) (void)hipFree(p); p = nullptr; cap = 0; owned = true; }
};

enum ProfClass { PC_GEMM_A1 = 0, PC_GEMM_A2 = 1, PC_GEMM_H = 2, PC_GEMM_J = 3, PC_SYR2K = 4, PC_KUF = 5, PC_POINT = 6, PC_RED = 7, PC_MXM = 8, PC_OTHER = 9 };

struct TileList {   // what a launch takes: a view of a device list that the tile cache owns (zigp_ctx::tiles)
  GemmTile* d = nullptr;
  int n = 0;     // list entries
  int per = 1;   // entries per workgroup (n is a multiple of it)
};
struct HipFree { void operator()(void* q) const { (void)hipFree(q); } };
struct CachedTiles {   // an entry of the tile cache: owns the device copy of its list
  std::unique_ptr<GemmTile, HipFree> d;
  int n = 0, per = 1;
  TileList view() const { return TileList{d.get(), n, per}; }
};

// Per-latent (f or g) device state of the dense path
struct Latent {
  int M = 0, Mp = 0;
  DevBuf Z, ell, u, s, s2;              // Z (Mp,D) zero padded; u,s,s2 (Mp) zero padded
  double zc[64] = {0};                       // [ZIGP_MAX_D] mean inducing input (host copy): centre of k_kgrad's moment sums
  bool kg_exact = false;                     // inducing inputs spread over > KG_EXACT_SPREAD lengthscales: k_kgrad forms x - z_m per row (no centre shift)
  DevBuf Zs;                            // Z scaled by KUF_C / ell_d (k_kuf_build's units), same padding
  double var = 1.0;
  DevBuf Kuu, L, W;                      // (Mp,Mp)
  DevBuf K, A1, Jp;                      // chunk panels [Mp][Nc]: Kuf, A1 = W K, J' = Q W^T A1 (A2 = W^T A1 is reduced to its column sums and never stored: r6)
  DevBuf Kd;                             // chunk panel [Mp][Nc] of a Matern latent's gradient step: K' = -dk / d(r2 / 2) (k_kuf_build_matern); freed when the latent goes back to RBF
  DevBuf Wp, a1gm;                       // W diag(s^2) (Mp,Mp); running sum of A1 gm [Mp]
  DevBuf Wt;                             // W^T (Mp,Mp): the m-contiguous image the lower-triangular product A1 = W K reads
  DevBuf P, Qt, Rt;                      // gradient steps: P = W^T W = Kuu^-1, Qt = diag(s^2) P - I = Q^T, Rt = W Qt = (Q W^T)^T: J' = Q A2 = (Q W^T) A1 (zigp_dense.hip, chunk_forward)
  bool P_ready = false;                  // P of THIS call's parameters is in `P` (the reverse M x M stage takes it from there)
  DevBuf part;                           // [3][Mp/32][Nc] partial rows of the fused column sums: v^T A1, sum A1^2, sum s^2 A2^2
  DevBuf gm, gv;                         // cotangents of mean / var per column [Nc]
  DevBuf du, dsq, krow;                  // row accumulators: du[Mp], dsq[Mp], krow[Mp][1+2D]
  DevBuf xm, mom, ks0;                   // wide Kuf gradient (D > 8, centred form): operand XM [Nc][128], split-K planes [S][Mp][128], per-split sum T [KG_SPLIT][Mp]
  DevBuf dLpart;                         // [S][Mp*Mp] split-K partials of the rank-N updates
  DevBuf T1, T2, T3, G;                  // MxM scratch
  DevBuf sk;                             // [S][Mp*Mp] split-K planes of the O(M^3) products of the reverse pass
  DevBuf vec;                            // small vectors: v=W u [Mp], alpha [Mp], dkinv [Mp], scal[8]
  DevBuf wh;                             // whitened calls (k_kl_white): s^2 - 1 [Mp], u [Mp], 1 [Mp], KL -- vec's layout as k_dense_pack reads it
  DevBuf Lraw, Lq, lqssq, dLq;           // full-covariance calls (zigp_set_q_full): the caller's (M,M) block, its masked padded image (Mp,Mp), k_lq_stage's
                                         // block sums [Mp*Mp/256], the gradient block (Mp,Mp); T - I lives in `P`, its image R^T = (T - I) W in `Rt`
};

struct KronState;   // Kronecker-path buffers (zigp_kron.hip)
struct KfState;     // fused Kronecker path (zigp_kronf.hip)

// Page-locked host staging for the small per-step transfers (parameters in, sums and gradients out).  A copy between
// device and PAGEABLE host memory makes the runtime stage and wait; through this arena the H2D copies are truly
// asynchronous and all D2H results of a call are collected by its single final stream synchronisation.  Blocks are never
// moved or freed while a call is in flight: alloc() only appends, reset() (start of every API call -- the previous
// call ended with a synchronisation) rewinds.
struct PinnedArena {
  struct Block { char* p; size_t cap, used; };
  std::vector<Block> blocks;
  PinnedArena() = default;
  PinnedArena(const PinnedArena&) = delete;
  PinnedArena& operator=(const PinnedArena&) = delete;
  ~PinnedArena() { for (auto& b : blocks) (void)hipHostFree(b.p); }
  void reset() { for (auto& b : blocks) b.used = 0; }
  void* alloc(size_t bytes) {
    bytes = (bytes + 63) & ~(size_t)63;
    for (auto& b : blocks)
      if (b.cap - b.used >= bytes) { void* r = b.p + b.used; b.used += bytes; return r; }
    Block nb; nb.cap = bytes > ((size_t)1 << 20) ? bytes : ((size_t)1 << 20); nb.used = bytes; nb.p = nullptr;
    if (hipHostMalloc((void**)&nb.p, nb.cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    blocks.push_back(nb);
    return nb.p;
  }
};

// The context's streams, events and Cholesky status word.  zigp_ctx derives from this and base classes are destroyed after the
// members, so every buffer of the context (its DevBufs, the tile cache, the Kronecker states) is freed before the streams go.
struct CtxHandles {
  hipStream_t stream = nullptr;    // stream every launch helper enqueues on (switched for a scope by OnStream)
  hipStream_t stream_main = nullptr, stream2 = nullptr;
  hipStream_t stream3 = nullptr;   // dense path: buffers, zeroed accumulators and the first chunk's Kuf panels, under the M x M forward of both latents
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_prep_fork = nullptr, ev_prep = nullptr;
  int* d_info = nullptr;
  struct PendingEv { hipEvent_t a, b; int cls; };
  std::vector<PendingEv> pending;       // profiling event pairs not yet read (prof_collect)
  std::vector<hipEvent_t> ev_pool;
  CtxHandles() = default;
  CtxHandles(const CtxHandles&) = delete;
  CtxHandles& operator=(const CtxHandles&) = delete;
  ~CtxHandles() {
    if (d_info) (void)hipFree(d_info);
    for (auto& e : pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ev_fork, ev_join, ev_prep_fork, ev_prep})
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {stream3, stream2, stream_main})
      if (s) (void)hipStreamDestroy(s);
  }
};

}  // namespace zigp

struct zigp_ctx : zigp::CtxHandles {
  ~zigp_ctx();                          // zigp_kron.hip, where KronState and KfState are complete
  int device = 0;
  std::string err;
  int info = 0;
  int64_t fit_steps_applied = 0;       // zigp_kron_fit_steps / zigp_kron_head_fit_steps: updates applied by the LAST call (all of them, or the ones before a failing step)
  int64_t chunk = 32768;
  bool chunk_auto = true;                // no zigp_set_chunk yet: the chunk follows M (32768 rows at M = 1024, more for smaller M)
  // data
  const double* dX = nullptr; const double* dY = nullptr;
  zigp::DevBuf ownX, ownY;
  int64_t N = 0; int D = 0;
  // zigp_select_rows: the active data (dX, dY, N) is a gathered batch of the resident set (fullX, fullY, fullN)
  const double* fullX = nullptr; const double* fullY = nullptr; int64_t fullN = 0;
  zigp::DevBuf selX, selY, selIdx;
  // zigp_fit_steps: the call's own gathered batch and row indices (the selection above is left as found), its device state
  // [x | m | v | history | failure record | hyperparameter block], and the updates its LAST call applied
  zigp::DevBuf fitX, fitY, fitIdx, fit;
  int64_t dense_fit_steps_applied = 0;
  // dense path state
  zigp::Latent lat[2];
  zigp::DevBuf pw_part;                 // pointwise block partials
  // mean function of f, m(x) = mean_b + mean_a . x (zigp_set_mean_function), and its gradient from the last zigp_elbo
  bool fwd_kuf_side = true;             // value-only / predict passes: the next chunk's Kuf panels on the side stream behind this chunk's A1 (env ZIGP_FWD_KUF_SIDE=0: off)
  bool trmm_tail = true;                // merged triangular launches: re-deal the last, partly filled wave (trmm_tiles, zigp_host.h); env ZIGP_TRMM_TAIL=0 turns it off
  int overlap = 1;                      // zigp_set_overlap: 1 (default) = HBM-bound side kernels of a chunk on stream2 under its SYRKs
  bool mean_on = false;
  bool whiten = false;                  // zigp_set_whiten: u_*m / u_*s_sqrt are the whitened quantities, q(u) = N(L u, L diag(s^2) L^T)
  int kern[2] = {0, 0};                 // zigp_set_kernel: ZIGP_KERN_* of latent f, g (dense path)
  bool q_full = false;                  // zigp_set_q_full (needs whiten): u_*s_sqrt are (M,M) lower-triangular factors Lq, q(u) = N(L u, L Lq Lq^T L^T)
  double mean_a[8] = {0}, mean_b = 0.0, mean_da[8] = {0}, mean_db = 0.0;   // 8 = zigp::MAXD (zigp_kernels.h)
  zigp::DevBuf out9;                    // predict outputs (9,Nc)
  zigp::DevBuf scratch, scratch2;       // misc
  zigp::DevBuf path_tab, path_out;      // sample paths (zigp_paths.hip): the call's tables and work matrices; the staged (nlat, S, N) result of a host call
  zigp::PinnedArena pinned;             // host staging of the per-step transfers
  std::unique_ptr<zigp::KronState> kron;
  std::unique_ptr<zigp::KfState> kronf;
  bool kron_panels = false;             // zigp_set_kron_panels: force the panel (GEMM-core) Kronecker path
  int kron_kern[2][2] = {{0, 0}, {0, 0}};   // zigp_set_kron_kernel: ZIGP_KERN_* of [latent f, g][factor 0, 1]; any Matern factor routes a call to the panel path ...
  bool kron_matern_fused = false;       // ... unless zigp_set_kron_matern_fused is on: then a fused-eligible grid runs the _kinds kernels of zigp_kronf.hip
  int kron_range_tiles = 1024;          // larger-grid fused backward: rows go through in ranges of this many 16-point tiles (bounded operand spill; zigp_set_kron_range_tiles)
  std::map<std::string, zigp::CachedTiles> tiles;   // tile lists by key (get_tiles, zigp_host.h); kept until zigp_destroy (bound: chunk_plan)
  // data-parallel exchange (zigp_comm_init): RCCL communicator, one rank per context / GPU
  void* comm = nullptr; int comm_rank = 0, comm_nranks = 1; int64_t comm_calls = 0;
  double comm_timeout_s = 120.0;         // zigp_comm_set_timeout: how long zigp_comm_init waits for its peers
  zigp::DevBuf packed;                  // result vector of the dense path (k_dense_pack)
  zigp::DevBuf parm;                    // parameters of both latents, one staged image (latents_upload); lat[h].Z / ell / u / s are views into it
  double pivot_rtol = 8.0;              // zigp_set_pivot_rtol: a Cholesky pivot <= pivot_rtol * eps * (variance + jitter) is ZIGP_ENOTPD
  // profiling
  bool prof_on = false;
  int prof_every = 8;                    // chunk-loop launches are timed on every prof_every-th chunk (event pairs cost ~10 us)
  bool prof_skip = false;                // set by the chunk loop for the chunks that are not sampled
  int64_t prof_total[ZIGP_NCLASS] = {0}; // all launches per class, sampled or not
  double prof_ms[ZIGP_NCLASS] = {0};
  int64_t prof_n[ZIGP_NCLASS] = {0};
  double prof_flops[ZIGP_NCLASS] = {0};
};

namespace zigp {

#define ZIGP_HIP(ctx, expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      char _b[512];                                                                      \
      snprintf(_b, sizeof(_b), "HIP error '%s' at %s:%d (%s)", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
      (ctx)->err = _b;                                                                   \
      return ZIGP_EHIP;                                                                  \
    }                                                                                    \
  } while (0)

#define ZIGP_TRY(expr)            \
  do {                            \
    int _rc = (expr);             \
    if (_rc != 0) return _rc;     \
  } while (0)

#define ZIGP_ENSURE(ctx, buf, n)                                        \
  do {                                                                  \
    if ((buf).ensure((size_t)(n)) != 0) {                               \
      (ctx)->err = "hipMalloc failed for " #buf;                        \
      return ZIGP_EHIP;                                                 \
    }                                                                   \
  } while (0)

inline int fail_arg(zigp_ctx* c, const char* msg) { c->err = msg; return ZIGP_EARG; }

// The stream the launch helpers enqueue on (c->stream), switched for one scope: restored on every exit path.
struct OnStream {
  zigp_ctx* c;
  hipStream_t saved;
  OnStream(zigp_ctx* c_, hipStream_t s) : c(c_), saved(c_->stream) { c->stream = s; }
  ~OnStream() { c->stream = saved; }
  OnStream(const OnStream&) = delete;
  OnStream& operator=(const OnStream&) = delete;
};

// Fork: `side` waits for what the main stream has enqueued so far (ev is recorded on the main stream).
inline int fork_side(zigp_ctx* c, hipEvent_t ev, hipStream_t side) {
  ZIGP_HIP(c, hipEventRecord(ev, c->stream_main));
  ZIGP_HIP(c, hipStreamWaitEvent(side, ev, 0));
  return 0;
}
// Join: the main stream waits for what `side` has enqueued so far (ev is recorded on `side`).
inline int join_side(zigp_ctx* c, hipEvent_t ev, hipStream_t side) {
  ZIGP_HIP(c, hipEventRecord(ev, side));
  ZIGP_HIP(c, hipStreamWaitEvent(c->stream_main, ev, 0));
  return 0;
}

// RAII-less profiling bracket: call prof_begin before and prof_end after a group of launches.
struct ProfScope {
  zigp_ctx* c; hipEvent_t a = nullptr, b = nullptr; int cls; bool on;
  static hipEvent_t get_ev(zigp_ctx* c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; return e;
  }
  ProfScope(zigp_ctx* c_, int cls_, double flops = 0.0) : c(c_), cls(cls_), on(c_->prof_on) {
    if (!on) return;
    c->prof_total[cls] += 1;
    if (c->prof_skip) { on = false; return; }
    a = get_ev(c); b = get_ev(c);
    if (!a || !b) { on = false; return; }
    (void)hipEventRecord(a, c->stream);
    c->prof_flops[cls] += flops;
    c->prof_n[cls] += 1;
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({a, b, cls});
  }
};

inline void prof_collect(zigp_ctx* c) {
  for (auto& p : c->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) c->prof_ms[p.cls] += ms;
    c->ev_pool.push_back(p.a); c->ev_pool.push_back(p.b);
  }
  c->pending.clear();
}

}  // namespace zigp
