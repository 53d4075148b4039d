// The call record of the Kronecker path and the host pieces its two routes share (zigp_kron.hip: the GEMM-panel path; zigp_kronf.hip:
// the fused kernels).  DESIGN.md section 7.  Host code only; everything is `static`, as in zigp_host.h.
#pragma once
#include "zigp_host.h"

namespace zigp {

// one latent's parameters as the host holds them (zigp_kron_params, per factor q = 0, 1)
// kind[q]: the factor's ZIGP_KERN_* (zigp_set_kron_kernel; kron_set_kinds fills it from the context, 0 = RBF otherwise)
struct KronHostLatent { int M[2]; const double* Z[2]; const double* ell[2]; double var[2]; const double* u; const double* s; int kind[2]; };

// One ELBO step or prediction: filled by the entry points (zigp_kron.hip; fields they do not set are zero), read by kron_run,
// kron_run_panels, kronf_run and kron_predict_chunked.
struct KronCall {
  // ---- inputs
  const zigp_kron_params* p;
  const double *X, *Y;          // N rows; Y nullptr: predict
  int64_t N;
  bool dev_xy;                  // X / Y are DEVICE pointers into the resident data set (zigp_set_data): nothing but the parameters is staged
  double jitter, scale;
  double g_offset;              // added to gmean before the probit moments (onofftf/onoffpred.py:141)
  double f_mu;                  // constant added to fmean (scripts/onoff.py:168-169, classifier.py:136-137); its gradient (the sum of the
                                // fmean cotangents) goes to *d_offset
  int include_kl;
  bool predict;
  int lik;
  // ---- outputs (any may be nullptr)
  double* out;                  // predict: [9][N] (on/off) or [4][N] (heads)
  double *elbo_data, *kl;
  zigp_kron_grads* grads;
  double* d_offset;
  // ---- derived (kron_call_derive)
  int nlat;                     // single-latent heads use the f latent only
  bool need_grad;
  KronHostLatent hl[2];         // nlat == 1: hl[1] = hl[0], the buffers that stand in for g
};

static void kron_host_latents(const zigp_kron_params* p, int nlat, KronHostLatent* hl) {
  hl[0] = {{p->M0f, p->M1f}, {p->Z0f, p->Z1f}, {p->ell0f, p->ell1f}, {p->var0f, p->var1f}, p->u_fm, p->u_fs_sqrt};
  hl[1] = {{p->M0g, p->M1g}, {p->Z0g, p->Z1g}, {p->ell0g, p->ell1g}, {p->var0g, p->var1g}, p->u_gm, p->u_gs_sqrt};
  if (nlat == 1) hl[1] = hl[0];
}

// the derived fields of a record whose inputs and outputs are set (p validated, or carrying the sizes only: a fit call)
static void kron_call_derive(KronCall& k) {
  k.nlat = (k.lik == ZIGP_LIK_ONOFF) ? 2 : 1;
  k.need_grad = k.grads != nullptr && !k.predict;
  kron_host_latents(k.p, k.nlat, k.hl);
}

// The factor kinds of a call: context state (zigp_set_kron_kernel), read once per call next to kron_call_derive.  A head (nlat == 1)
// follows the f kinds.
static void kron_set_kinds(const zigp_ctx* c, KronHostLatent* hl, int nlat) {
  for (int h = 0; h < 2; ++h)
    for (int q = 0; q < 2; ++q) hl[h].kind[q] = c->kron_kern[nlat == 1 ? 0 : h][q];
}
static const char* kron_kern_name(int kind) { return kind == ZIGP_KERN_MATERN32 ? "Matern32" : kind == ZIGP_KERN_MATERN52 ? "Matern52" : "RBF"; }
// "<kernel> kernel on factor <q> of latent <f|g>" of the first Matern factor of the call's latents, or empty: every factor is RBF
static std::string kron_matern_factor(const KronHostLatent* hl, int nlat) {
  for (int h = 0; h < nlat; ++h)
    for (int q = 0; q < 2; ++q)
      if (hl[h].kind[q] != ZIGP_KERN_RBF)
        return std::string(kron_kern_name(hl[h].kind[q])) + " kernel on factor " + std::to_string(q) + " of latent " + (h ? "g" : "f");
  return std::string();
}

// what a Cholesky failure names: one job of the fused factor kernel, or (predictions, the panel path) the factors as a whole
static const char* const kron_fac_names[4] = {"Kronecker factor 0 of Kuu (latent f)", "Kronecker factor 1 of Kuu (latent f)",
                                              "Kronecker factor 0 of Kuu (latent g)", "Kronecker factor 1 of Kuu (latent g)"};
static const char* const kron_fac_any = "a Kronecker factor of Kuu";

// KL from the five scalars per latent (klv[h]: sum U.Alpha, sum log s^2, the diag(P0) diag(P1) s^2 sum, logdet K0, logdet K1).  In a
// data-parallel run of the fused path they are sums over the ranks that count the KL -- kl_ranks of them: one, by the contract of
// zigp_comm_init -- and every rank returns the same value; the panel path passes 1 (or 0: not counted).  k_fit_update holds the device's copy.
static double kron_kl(const KronCall& k, const double* const* klv, double kl_ranks) {
  double klsum = 0.0;
  if (kl_ranks > 0.0) {
    for (int h = 0; h < k.nlat; ++h) {
      const double* v = klv[h];
      const int M0 = k.hl[h].M[0], M1 = k.hl[h].M[1];
      klsum += 0.5 * (v[0] - kl_ranks * (double)M0 * M1 - v[1] + v[2] + (double)M1 * v[3] + (double)M0 * v[4]);
    }
  }
  return klsum;
}

// k.grads from the downloaded pieces: krow[h][q] rows [M][2 + 2 D] (sum for d var | d Z numerators | d ell numerators), gu / gs [M0 M1],
// s_gv[h] the sum of the variance cotangents over the points, d_noise.  dZ = krow / ell^2, d ell = sum_m krow / ell^3 (m ascending),
// d var = sum_m krow / var + s_gv var_other.
static void kron_assemble_grads(const KronCall& k, const double* const (*krow)[2], const double* const* gu, const double* const* gs,
                                const double* s_gv, double d_noise) {
  zigp_kron_grads* g = k.grads;
  double* gZ[2][2] = {{g->Z0f, g->Z1f}, {g->Z0g, g->Z1g}};
  double* gl[2][2] = {{g->ell0f, g->ell1f}, {g->ell0g, g->ell1g}};
  double* gum[2] = {g->u_fm, g->u_gm};
  double* gus[2] = {g->u_fs_sqrt, g->u_gs_sqrt};
  double gvar[2][2] = {{0, 0}, {0, 0}};
  for (int h = 0; h < k.nlat; ++h) {
    const KronHostLatent& L = k.hl[h];
    for (int q = 0; q < 2; ++q) {
      const int D = q == 0 ? k.p->D0 : k.p->D1, W = 2 + 2 * D;
      const double* ell = L.ell[q];
      double dv = 0.0, dl[MAXD] = {0};
      for (int m = 0; m < L.M[q]; ++m) {
        const double* r = &krow[h][q][(size_t)m * W];
        dv += r[0];
        for (int d = 0; d < D; ++d) {
          if (gZ[h][q]) gZ[h][q][m * D + d] = r[1 + d] / (ell[d] * ell[d]);
          dl[d] += r[1 + D + d];
        }
      }
      for (int d = 0; d < D; ++d)
        if (gl[h][q]) gl[h][q][d] = dl[d] / (ell[d] * ell[d] * ell[d]);
      gvar[h][q] = dv / L.var[q] + s_gv[h] * L.var[1 - q];   // Knn = var0 * var1 enters var_n directly (scripts/onoff.py:196-200)
    }
    const size_t ng = (size_t)L.M[0] * L.M[1];
    if (gum[h]) memcpy(gum[h], gu[h], sizeof(double) * ng);
    if (gus[h]) memcpy(gus[h], gs[h], sizeof(double) * ng);
  }
  g->var0f = gvar[0][0]; g->var1f = gvar[0][1];
  g->var0g = gvar[1][0]; g->var1g = gvar[1][1];
  g->noise = d_noise;
}

}  // namespace zigp
