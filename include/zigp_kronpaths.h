/* Kronecker sample paths: joint posterior draws at test inputs for the Kronecker (space x time) model and its single-latent heads
 * (DESIGN.md section 10e).  Part of the C boundary of libzigp.so: include/zigp.h includes this file behind the sample paths of the dense
 * model, whose zigp_path_draw record and ZIGP_PATH_MAX_S it uses -- include zigp.h, not this file. */
#ifndef ZIGP_KRONPATHS_H
#define ZIGP_KRONPATHS_H

/* A product of two RBF factors is an RBF over the D0 + D1 columns, so a path of the Kronecker model is the sum above over the M0 M1 grid
 * points -- but a row needs only M0 + M1 factor values, and every grid-point feature is one multiply.  Per latent h, row n and sample s,
 * THE definition:
 *   out[h][s][n] = shift_h + sum_{i<M0} sum_{j<M1} V_h[i M1 + j][s] ( k0_h(x_n[0:D0], z0_i) k1_h(x_n[D0:D0+D1], z1_j) )
 *                + sum_{r<R} amp_h[r][s] cos( sum_{d<D0+D1} omega_h[r][d] x[n][d] + phase_h[r] )
 * k_q(x, z) = var_q exp(-1/2 sum_d ((z_d - x_d) / ell_q,d)^2) with the element function of zigp_kron_predict's factor panels; the product
 * k0 k1 is rounded once; V is factor-0-major, as u_fm is.  One summation order per element (groups of four grid points with one i, ascending
 * j inside ascending i, M1 padded to a multiple of 4 by zero weights; then the cosines in ascending r; shift last): an element's bits do not
 * depend on N, on the row's position, on S, on the sample's column, on the other latent or on the call.
 * Each factor has its own kernel family: the record's fourth word (it keeps its name, `reserved`) holds the kinds = kind0 + 4 * kind1 of two
 * ZIGP_KERN_* values (0, what every caller has passed so far, is RBF x RBF as above).  A Matern factor evaluates k_q with the element function of its own factor panel (zigp_set_kron_kernel): the same
 * r2 -- fused multiply-adds from 0 in ascending d of (z_d / ell_d - x_d / ell_d) -- then r = sqrt(r2 + 1e-12) and
 *   ZIGP_KERN_MATERN32  k_q = var_q (1 + sqrt3 r) exp(-sqrt3 r),     ZIGP_KERN_MATERN52  k_q = var_q (1 + sqrt5 r + (5/3) r^2) exp(-sqrt5 r).
 * The product of a Matern factor with any other is not a stationary kernel of one distance, but its spectral density is the product of
 * the factors' densities: the frequencies of factor q's columns follow that factor's law (zigp.pathwise.kron_draw).
 * ZIGP_EARG with a message that names the argument, nothing enqueued and the context usable afterwards: D0 or D1 < 1, D0 + D1 > 8, M0 or M1
 * outside [1, 128], kinds outside the nine valid values, S outside [1, ZIGP_PATH_MAX_S], R < 0, a NULL table, a non-finite table entry, a host pointer handed to a _device call. */
typedef struct {
  int32_t M0, M1, R, reserved;       /* inducing points of factor 0 and 1, random features; reserved carries the KINDS: kind0 + 4 * kind1 (0: RBF x RBF) */
  const double* Z0;                  /* (M0,D0) */
  const double* Z1;                  /* (M1,D1) */
  const double* ell0;                /* (D0) */
  const double* ell1;                /* (D1) */
  double var0, var1;
  const double* V;                   /* (M0*M1,S) weights of the grid points, row i*M1 + j */
  const double* omega;               /* (R,D0+D1) frequencies */
  const double* phase;               /* (R) */
  const double* amp;                 /* (R,S) weights of the cosines */
  double shift;
} zigp_kron_path_latent;
/* The sum above and nothing else.  lat: nlat (1 or 2) records -- the two latents may have different grids -- all arrays in host memory;
 * X (N,D0+D1) and out (nlat,S,N) in host memory. */
int zigp_kron_path_rows(zigp_ctx* ctx, const zigp_kron_path_latent* lat, int32_t nlat, int32_t D0, int32_t D1, int32_t S, const double* X,
                        int64_t N, double* out);
/* The same with X and out in DEVICE memory of the context's GPU (the tables stay host pointers); complete on return. */
int zigp_kron_path_rows_device(zigp_ctx* ctx, const zigp_kron_path_latent* lat, int32_t nlat, int32_t D0, int32_t D1, int32_t S, const double* dX,
                               int64_t N, double* d_out);
/* Joint sample paths of the Kronecker OnOff model.  The draws are zigp_path_draw records with omega0 (R,D0+D1) and eps (M0*M1,S).  Per
 * latent: omega = omega0 / [ell0 | ell1], amp = a sqrt(2 var0 var1 / R); f_Z = the sum above at the M0 M1 grid points (i, j) with V = 0;
 * rhs_s = U + S o E_s - F_Z,s as M0 x M1 matrices; V_s = K0^-1 rhs_s K1^-1, formed as W0^T (W0 rhs_s W1^T) W1 with the W_p = L_p^-1 of the
 * call's own factor forward stage (K_p + jitter I = L_p L_p^T, the one zigp_kron_predict runs); then the sum at Xnew with f_mu as the shift of f and g_offset as the shift of g, as rows fmean and gmean
 * of zigp_kron_predict carry them.  out3 is (3,S,N): f, g, and gf = Phi~(g) f with the link of the predictive density.
 * The factor kinds are the context's (zigp_set_kron_kernel; the heads follow the f kinds): the factor forward stage and the sum evaluate
 * the same k_q.  zigp_kron_predict's errors (ZIGP_ENOTPD names the factors) and the refusals above. */
int zigp_kron_sample_paths(zigp_ctx* ctx, const zigp_kron_params* p, const double* Xnew, int64_t N, double jitter, double g_offset, double f_mu,
                           const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* out3);
/* The same with Xnew and out3 in DEVICE memory of the context's GPU; the draws stay host pointers; complete on return. */
int zigp_kron_sample_paths_device(zigp_ctx* ctx, const zigp_kron_params* p, const double* dXnew, int64_t N, double jitter, double g_offset,
                                  double f_mu, const zigp_path_draw* draw_f, const zigp_path_draw* draw_g, int32_t S, double* d_out3);
/* Sample paths of a single-latent head (only the f fields of p are read).  ZIGP_LIK_GAUSSIAN: out is (1,S,N), f + f_mu.
 * ZIGP_LIK_BERNOULLI: out is (2,S,N), f + f_mu and the probability Phi~(f + f_mu) -- the reference's probit link with its 1e-3 clamp
 * (scripts/classifier.py:216-217). */
int zigp_kron_head_sample_paths(zigp_ctx* ctx, const zigp_kron_params* p, int32_t lik, const double* Xnew, int64_t N, double jitter, double f_mu,
                                const zigp_path_draw* draw_f, int32_t S, double* out);
int zigp_kron_head_sample_paths_device(zigp_ctx* ctx, const zigp_kron_params* p, int32_t lik, const double* dXnew, int64_t N, double jitter,
                                       double f_mu, const zigp_path_draw* draw_f, int32_t S, double* d_out);

#endif
