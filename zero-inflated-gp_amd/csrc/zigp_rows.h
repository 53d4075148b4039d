// The host layer of a "row call": an entry that takes predictive rows -- the caller's, or those of a predict block it runs itself -- and
// puts one row-wise kernel over them (zigp_density.hip, zigp_score.hip, zigp_paths.hip; zigp_predict is the block alone).  DESIGN.md
// section 10d.  Host code and the one kernel that adds block partials; everything is `static`, as in zigp_host.h.
//
// A row call enqueues on c->stream, in this order: the staging copies (stage_inputs, rows_from_host), run_dense in predict mode
// (rows_from_predict; complete on return), the rule's table (upload_rule), its rows kernel, the sum of the block partials (sum_partials),
// the copies to the host and the one synchronisation (finish_copies).  Its device regions come from a RowArena over a buffer of the
// context and are dead after that synchronisation: no call reads what an earlier one left there, so every call's regions start at 0.
#pragma once
#include "zigp_host.h"

namespace {
int run_dense(zigp_ctx* c, const zigp_params* p, const double* dX, const double* dY, int64_t Nrows, int D, double jitter, double scale,
              double g_offset, int64_t row_begin, int64_t row_end, int include_kl, bool predict, double* d_out9, double* elbo_data,
              double* kl, zigp_grads* grads);   // zigp_dense.hip
}

namespace zigp {

// ZIGP_EARG with the message "<who>: <what>"
static int refuse(zigp_ctx* c, const std::string& who, const std::string& what) { return fail_arg(c, (who + ": " + what).c_str()); }

// Regions of one DevBuf in allocation order, each starting on a multiple of 8 doubles: take() every region, commit() once (the only
// allocation), then at().  name: the buffer as an allocation failure names it.
struct RowArena {
  DevBuf& buf;
  const char* name;
  size_t total = 0;
  RowArena(DevBuf& b, const char* nm) : buf(b), name(nm) {}
  size_t take(size_t n) { const size_t r = (total + 7) & ~(size_t)7; total = r + n; return r; }
  int commit(zigp_ctx* c) {
    if (buf.ensure(total) == 0) return 0;
    c->err = std::string("hipMalloc failed for ") + name;
    return ZIGP_EHIP;
  }
  double* at(size_t r) const { return buf.p + r; }
};

// Host rows X (N, D) and -- where there are any -- Y (N) into scratch, Y from the next multiple of 8 doubles; device rows as they are
static int stage_inputs(zigp_ctx* c, const double* X, int64_t N, int D, bool on_device, const double** dX, const double* Y = nullptr,
                        const double** dY = nullptr) {
  if (!on_device) {
    RowArena in(c->scratch, "c->scratch");
    const size_t ox = in.take((size_t)N * D), oy = in.take(Y ? (size_t)N : 0);
    ZIGP_TRY(in.commit(c));
    ZIGP_HIP(c, hipMemcpyAsync(in.at(ox), X, sizeof(double) * N * D, hipMemcpyHostToDevice, c->stream));
    if (Y) ZIGP_HIP(c, hipMemcpyAsync(in.at(oy), Y, sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    X = in.at(ox);
    if (Y) Y = in.at(oy);
  }
  *dX = X;
  if (dY) *dY = Y;
  return 0;
}

// The rows a row-wise kernel reads, all device pointers: fm, fv, gm, gv (rows 3-6 of a predict block; gm, gv OnOff only), y (nullable)
// and -- a predict block -- m0, m1, m2 = its gfmean, gfvar, gfmeanu, else NULL
struct PredRows {
  const double* fm; const double* fv; const double* gm; const double* gv; const double* y;
  const double* m0; const double* m1; const double* m2;
  int64_t N;
};

// The caller's host rows, staged into scratch as [fm | fv | y | gm | gv] (gm, gv: OnOff only; a NULL y is left out)
static int rows_from_host(zigp_ctx* c, bool onoff, const double* fm, const double* fv, const double* gm, const double* gv, const double* y,
                          int64_t N, PredRows& r) {
  ZIGP_ENSURE(c, c->scratch, (size_t)5 * N);
  double* d = c->scratch.p;
  const double* src[5] = {fm, fv, y, gm, gv};
  for (int k = 0; k < (onoff ? 5 : 3); ++k)
    if (src[k]) ZIGP_HIP(c, hipMemcpyAsync(d + k * N, src[k], sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
  r = PredRows{d, d + N, onoff ? d + 3 * N : nullptr, onoff ? d + 4 * N : nullptr, y ? d + 2 * N : nullptr, nullptr, nullptr, nullptr, N};
  return 0;
}

// The rows of a predict block at X (N, D) with the targets Y (N, nullable), both the host's or -- on_device -- device memory: out9 of
// run_dense, which is complete on return
static int rows_from_predict(zigp_ctx* c, const zigp_params* p, const double* X, const double* Y, int64_t N, double jitter, double g_offset,
                             bool on_device, PredRows& r) {
  ZIGP_TRY(stage_inputs(c, X, N, p->D, on_device, &X, Y, &Y));
  ZIGP_ENSURE(c, c->out9, (size_t)9 * N);
  ZIGP_TRY(run_dense(c, p, X, nullptr, N, p->D, jitter, 1.0, g_offset, 0, N, 0, true, c->out9.p, nullptr, nullptr, nullptr));
  const double* o = c->out9.p;
  r = PredRows{o + 3 * N, o + 4 * N, o + 5 * N, o + 6 * N, Y, o, o + N, o + 2 * N, N};
  return 0;
}

// Where a kernel writes an optional output: nowhere (NULL), the caller's device memory, or the call's staging slot
static inline double* out_target(double* out, bool on_device, double* slot) { return !out ? nullptr : on_device ? out : slot; }

// The caller's rule for N(0, 1) as the table a rows kernel reads: the nodes x, then a column of the weights, then -- one form -- x^2 / 2
enum class RuleForm { X_LOGW, X_LOGW_HALFX2, X_W };
static int upload_rule(zigp_ctx* c, double* dst, const double* nodes, const double* weights, int n_quad, RuleForm form) {
  const int nq = n_quad, cols = form == RuleForm::X_LOGW_HALFX2 ? 3 : 2;
  ZIGP_PINNED(c, h, cols * (size_t)nq);
  for (int i = 0; i < nq; ++i) {
    h[i] = nodes[i]; h[nq + i] = form == RuleForm::X_W ? weights[i] : log(weights[i]);
    if (cols == 3) h[2 * nq + i] = 0.5 * nodes[i] * nodes[i];
  }
  ZIGP_HIP(c, hipMemcpyAsync(dst, h, sizeof(double) * cols * nq, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// One block: thread t adds the partials t, t + SUM_THREADS, ... in that order, then the threads' sums are added in thread order --
// the same association on every call, so the sum is bit-stable.
constexpr int SUM_THREADS = 256;
__global__ void __launch_bounds__(SUM_THREADS)
k_sum_partials(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double sh[SUM_THREADS / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += SUM_THREADS) s += part[b];
  s = block_sum<SUM_THREADS / 64>(s, sh);
  if (threadIdx.x == 0) out[0] = s;
}

// The nb block partials into dsum[0]; *hsum holds the sum after the call's synchronisation
static int sum_partials(zigp_ctx* c, const double* part, int nb, double* dsum, double** hsum) {
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(SUM_THREADS), 0, c->stream, part, nb, dsum);
  ZIGP_HIP(c, hipGetLastError());
  return download(c, dsum, 1, hsum);
}

// The end of a row call: the copies to the host (dst NULL: that output was not asked for, or lives on the device), then the stream's
// synchronisation
struct RowCopy { double* dst; const double* src; size_t n; };   // host, device, doubles
static int finish_copies(zigp_ctx* c, std::initializer_list<RowCopy> copies) {
  for (const RowCopy& k : copies)
    if (k.dst) ZIGP_HIP(c, hipMemcpyAsync(k.dst, k.src, sizeof(double) * k.n, hipMemcpyDeviceToHost, c->stream));
  ZIGP_HIP(c, hipStreamSynchronize(c->stream));
  return ZIGP_OK;
}

}  // namespace zigp
