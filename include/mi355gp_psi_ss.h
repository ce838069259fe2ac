/* mi355gp_psi_ss.h -- psi-statistics of the RBF kernel for spike-and-slab inputs
 *   q(x_nq) = gamma_nq N(mu_nq, S_nq) + (1 - gamma_nq) delta_0
 * and their gradients (csrc/psi_ss.hip; GPy/kern/src/psi_comp/ssrbf_psi_comp.py, ssrbf_psi_gpucomp.py).  A header of its own
 * next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table PSI_SS_ABI, which tests/test_oracle_psi_ss.py holds against
 * the prototypes here.  The first two calls are stateless: they upload, compute and download.  Every sum is combined in a fixed order
 * (no floating-point atomics): two calls with the same arguments give the same bytes, and psi2 is bitwise symmetric. */
#ifndef MI355GP_PSI_SS_H
#define MI355GP_PSI_SS_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* psi1 (N x M) and / or psi2 = sum_n w_n psi2n (M x M); either output may be NULL.  lengthscale: D entries if ard, else one.
 * Z: M x D; mu, S, gamma: N x D, S positive, gamma strictly inside (0, 1) (a bad entry is refused with its row and column);
 * weights (N) may be NULL.  D > 64 is refused by name. */
int mi355gp_ssrbf_psi(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                      const double* mu, const double* S, const double* gamma, int64_t N, int D, const double* weights,
                      double* psi1_out, double* psi2_out);

/* The six gradients of sum dL_dpsi0 psi0 + sum dL_dpsi1 * psi1 + sum sym(dL_dpsi2) * psi2 (ssrbf_psi_comp.py:290-398).  Each of
 * dL_dpsi0 (N), dL_dpsi1 (N x M), dL_dpsi2 (M x M, symmetrised inside) may be NULL.  dl_out: D entries if ard, else one;
 * dZ_out M x D; dmu_out, dS_out, dgamma_out N x D.  Where a factor of psi1 / psi2 underflows to 0 the element contributes
 * exactly 0 to every gradient. */
int mi355gp_ssrbf_psi_grad(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                           const double* mu, const double* S, const double* gamma, int64_t N, int D, const double* weights,
                           const double* dL_dpsi0, const double* dL_dpsi1, const double* dL_dpsi2, double* dvar_out,
                           double* dl_out, double* dZ_out, double* dmu_out, double* dS_out, double* dgamma_out);

/* ---- the sparse context (mi355gp_sparse_create ... of mi355gp.h) with spike-and-slab inputs ---------------------------------- */

/* Slab probabilities gamma (N x D, the shape of set_data's X) next to the resident means and variances; input variances must
 * have been set.  gamma == NULL takes the context back to Gaussian inputs (N and D are then ignored).  Every entry must be
 * finite and strictly inside (0, 1): a bad entry is refused with its row and column.  mi355gp_sparse_set_data forgets them. */
int mi355gp_sparse_set_binary_prob(mi355gp_sparse* s, const double* gamma, int64_t N, int D);

/* The three-array form of mi355gp_sparse_set_inputs, the upload of one SSGPLVM step: X (the means), S and gamma, all N x D and
 * all required; Y and everything sized by it stay resident. */
int mi355gp_sparse_set_inputs_ss(mi355gp_sparse* s, const double* X, const double* S, const double* gamma, int64_t N, int D);

/* One VarDTC evaluation with spike-and-slab inputs: mi355gp_vardtc_inference_uncertain's parameters plus dgamma_out (optional,
 * N x D).  One RBF part (isotropic or ARD, any active_dims) alone or summed with White parts, one noise variance.  Refused by
 * name before any device work: a context without gamma, a row-sharded context, Bias, Linear and every other kind, products,
 * per-point noise, D > 64.  (mi355gp_vardtc_inference_uncertain in turn refuses a context WITH gamma.)  The result lies where
 * VarDTC's does: mi355gp_sparse_predict, mi355gp_sparse_fetch and mi355gp_sparse_predict_uncertain at Gaussian new points
 * serve it. */
int mi355gp_vardtc_inference_ss(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars, double* dtheta_out,
                                double* dZ_out, double* wv_out, double* dmu_out, double* dS_out, double* dgamma_out,
                                double* stage_ms);

#ifdef __cplusplus
}
#endif
#endif
