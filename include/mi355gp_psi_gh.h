/* mi355gp_psi_gh.h -- psi-statistics by Gauss-Hermite quadrature for the stationary kernels that have no closed form
 * (Matern52, Matern32, Exponential / OU; ExpQuad is taken too), and their gradients (csrc/psi_gh.hip; the computation of
 * GPy/kern/src/psi_comp/gaussherm.py).  With nodes t_i and weights w_i (hermgauss(H): t_i = sqrt(2) x_i, w_i = omega_i / sqrt(pi))
 * and X(i) = mu + t_i sqrt(S) -- the SAME node in every dimension, the reference's rule: for D > 1 this is not a tensor quadrature --
 *   psi0[n] = sum_i w_i Kdiag(X(i))[n],   psi1 = sum_i w_i K(X(i), Z),   psi2 = sum_i w_i K(X(i), Z)^T K(X(i), Z).
 * A header of its own next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table PSI_GH_ABI.  The first two calls are
 * stateless: they upload, compute and download.  Every sum is combined in a fixed order (no floating-point atomics): two calls with
 * the same arguments give the same bytes, and psi2 is bitwise symmetric. */
#ifndef MI355GP_PSI_GH_H
#define MI355GP_PSI_GH_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MI355GP_GH_HMAX 32     /* most quadrature nodes */

/* kind: MI355GP_RBF (ExpQuad), _MATERN52, _MATERN32 or _EXPONENTIAL; theta = [variance, lengthscale (D entries if ard, else one)].
 * Z: M x D; mu, S: N x D, every S positive and finite (a bad entry is refused with its row and column); nodes, weights: H entries,
 * 1 <= H <= 32.  psi0_out (N), psi1_out (N x M), psi2_out (M x M): each may be NULL.  D > 64 and M > 65535 are refused by name. */
int mi355gp_gh_psi(int device, int kind, int ard, const double* theta, const double* Z, int64_t M, const double* mu,
                   const double* S, int64_t N, int D, const double* nodes, const double* weights, int H, double* psi0_out,
                   double* psi1_out, double* psi2_out);

/* The gradients of sum dL_dpsi0 psi0 + sum dL_dpsi1 * psi1 + sum dL_dpsi2 * psi2 (gaussherm.py:60-101; dL_dpsi2 enters as
 * dL_dpsi2 + dL_dpsi2^T).  dL_dpsi0 (N), dL_dpsi1 (N x M) and dL_dpsi2 (M x M) may each be NULL.  dL_dpsi1 may instead be given in
 * the rank form beta R v^T of a VarDTC fit: rank_R (N x Dy), rank_v (M x Dy), Dy and beta, with dL_dpsi1 == NULL.  Outputs, each may
 * be NULL: dtheta_out in theta order, dZ_out M x D, dmu_out and dS_out N x D. */
int mi355gp_gh_psi_grad(int device, int kind, int ard, const double* theta, const double* Z, int64_t M, const double* mu,
                        const double* S, int64_t N, int D, const double* nodes, const double* weights, int H,
                        const double* dL_dpsi0, const double* dL_dpsi1, const double* rank_R, const double* rank_v, int Dy,
                        double beta, const double* dL_dpsi2, double* dtheta_out, double* dZ_out, double* dmu_out,
                        double* dS_out);

/* One VarDTC evaluation with uncertain inputs whose statistics come from the quadrature: mi355gp_vardtc_inference_uncertain's
 * phases, parameters and result record, plus the nodes and weights.  ONE stationary part of the four kinds above (isotropic or ARD,
 * any active_dims) alone or summed with White parts, one noise variance.  Refused by name before any device work: Bias, Linear and
 * every other kind, a second input-dependent part, products, per-point noise, a row-sharded context, a context that holds slab
 * probabilities or output groups, D > 64.  The result lies where VarDTC's does: mi355gp_sparse_predict and mi355gp_sparse_fetch
 * serve it; mi355gp_sparse_predict_uncertain does not (it is the closed form of the RBF kernel). */
int mi355gp_vardtc_inference_gh(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                const double* noise, int64_t noise_len, double extra_jitter, const double* nodes,
                                const double* weights, int H, double* out_scalars, double* dtheta_out, double* dZ_out,
                                double* wv_out, double* dmu_out, double* dS_out, double* stage_ms);

#ifdef __cplusplus
}
#endif
#endif
