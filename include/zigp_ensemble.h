/* Sample-path scores: group totals, their CRPS, the energy score and the variogram score of an ensemble against an observation
 * (DESIGN.md section 10f).  Part of the C boundary of libzigp.so: include/zigp.h includes this file behind the sample paths, whose
 * ZIGP_PATH_MAX_S it uses -- include zigp.h, not this file.  Replaces nothing the reference computes: its scripts log RMSE / MAE (and
 * accuracy / AUC) of the predictive mean only, so the finite sums below are THE definition. */
#ifndef ZIGP_ENSEMBLE_H
#define ZIGP_ENSEMBLE_H

/* An ensemble E[s][n] of S members by N rows (member s at E + s ld, ld >= N), an observation y[n], row weights a[n] >= 0 (NULL: all 1)
 * and G >= 1 groups of contiguous rows, group g = the rows off[g] <= n < off[g+1] with off[0] = 0, off[G] = N, off non-decreasing.
 * Member S is the observation, x_S = y.  With D_g(u, v) = sqrt( sum_{n in g} a_n (u_n - v_n)^2 ), per group:
 *   total[s][g]   = sum_{n in g} a_n E[s][n]  (s < S),      total_obs[g] = sum_{n in g} a_n y_n
 *   crps_total[g] = (1/S) sum_s |total[s][g] - total_obs[g]| - c sum_{s<t} |total[s][g] - total[t][g]|
 *   energy[g]     = (1/S) sum_s D_g(x_s, y)                  - c sum_{s<t} D_g(x_s, x_t)
 *   variogram[g]  = sum_{i<j in g} a_i a_j ( |y_i - y_j|^p - (1/S) sum_s |E[s][i] - E[s][j]|^p )^2,   p = vario_p in {0.5, 1, 2}
 *   dist[g]       = the (S+1, S+1) symmetric matrix of D_g, zero diagonal, member S = the observation
 * c = 1 / S^2, or 1 / (S (S - 1)) with fair = 1 (S = 1 is then refused).  An empty group is legal: all its outputs are +0.
 * Shapes: total (S, G), total_obs, crps_total, energy, variogram (G), dist (G, S+1, S+1).  Every output is optional: NULL is neither
 * computed nor charged.  The differences are formed first and squared (never a Gram form G_ss + G_tt - 2 G_st).
 * One summation order per output element (rows in chunks of ZIGP_ENS_CHUNK counted from the group's start, four
 * interleaved row classes per chunk, chunks in ascending order; no atomics): an element's bits do not depend on N, G, the group's place
 * in the array, ld, which other outputs were asked for, or the call.  Non-finite ensemble values are not searched for: they propagate.
 * ZIGP_EARG with a message that names the argument, nothing enqueued, the outputs untouched and the context usable afterwards: a NULL
 * context (before anything else is read), S outside [1, ZIGP_PATH_MAX_S], N outside [1, 2^31), ld < N, a NULL E, y or off, G < 1,
 * boundaries that do not start at 0, end at N or that decrease, fair outside {0, 1}, fair = 1 with S = 1, vario_p outside
 * {0, 0.5, 1, 2}, a variogram pointer with vario_p = 0 (or the reverse), a variogram group of more than ZIGP_ENS_VARIO_MAX_ROWS rows,
 * a negative or non-finite host weight (device weights are not read by the host), a host pointer handed to the _device call. */
#define ZIGP_ENS_CHUNK 64
#define ZIGP_ENS_VARIO_MAX_ROWS 4096
typedef struct {
  int32_t fair;      /* 0: c = 1 / S^2;  1: c = 1 / (S (S - 1)) */
  double vario_p;    /* 0.5, 1 or 2; 0 when no variogram is asked */
} zigp_ens_opts;
/* Everything in host memory; opts NULL: fair = 0, vario_p = 0.  The reference logs RMSE / MAE only (scripts/onoff.py). */
int zigp_ensemble_scores(zigp_ctx* ctx, const double* E, int64_t ld, int32_t S, int64_t N, const double* y, const double* a, const int64_t* off,
                         int32_t G, const zigp_ens_opts* opts, double* total, double* total_obs, double* crps_total, double* energy,
                         double* variogram, double* dist);
/* The same with E, y, a and the six outputs in DEVICE memory of the context's GPU -- E may be a plane of a (3, S, N) paths block, or a
 * row-strided view of one; off and opts stay host pointers; complete on return.  The reference logs RMSE / MAE only. */
int zigp_ensemble_scores_device(zigp_ctx* ctx, const double* dE, int64_t ld, int32_t S, int64_t N, const double* dy, const double* da,
                                const int64_t* off, int32_t G, const zigp_ens_opts* opts, double* d_total, double* d_total_obs,
                                double* d_crps_total, double* d_energy, double* d_variogram, double* d_dist);

#endif
