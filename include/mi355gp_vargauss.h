/* mi355gp_vargauss.h -- the variational Gaussian approximation of Opper and Archambeau (2009) on the exact context
 * (csrc/vargauss.hip; GPy/inference/latent_function_inference/var_gauss.py:28-69): q(f) = N(K alpha, (K^-1 + diag(beta^2))^-1)
 * for one output column.  A header of its own next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table VARGAUSS_ABI,
 * which tests/test_oracle_vargauss.py holds against the prototypes here.
 *
 * All three calls run inside a session that mi355gp_laplace_begin has opened (K = kern.K(X) resident).  After forward,
 * mi355gp_laplace_predict (woodbury_vector = alpha) and mi355gp_fetch of K and of the woodbury_inv serve the result; after
 * backward mi355gp_fetch serves dL_dK as well.  The likelihood's variational expectations are O(N) host work between the two.
 * A positive return value is a LAPACK-style info (the first non-positive pivot of A), a negative one an error
 * (mi355gp_last_error).  Two calls with the same inputs give the same bytes. */
#ifndef MI355GP_VARGAUSS_H
#define MI355GP_VARGAUSS_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* alpha, beta (N each; beta signed, every entry finite and not zero): A = I + diag(beta) K diag(beta) (+ extra_jitter on the
 * diagonal) is factored and inverted;  m_out = K alpha,  var_out = diag (K^-1 + diag(beta^2))^-1 = Kdiag - colsumsq(L_A^-1
 * diag(beta) K) (no cancellation),  scal_out[0..2] = log det A, tr A^-1, m^T alpha. */
int mi355gp_vargauss_forward(mi355gp_ctx* ctx, const double* alpha, const double* beta, double extra_jitter, double* m_out,
                             double* var_out, double* scal_out);

/* dF_dm, dF_dv (N each, finite): dalpha_out = K dF_dm - m,  dbeta_out = dF_db - dKL_db (var_gauss.py:48-60), and dtheta_out =
 * every part's dL/dtheta (concatenated, as mi355gp_laplace_gradients') from the symmetrised (dL_dK + dL_dK^T) / 2 of :63-65,
 * which stays on the device for mi355gp_fetch(MI355GP_FETCH_DLDK).  Once per forward. */
int mi355gp_vargauss_backward(mi355gp_ctx* ctx, const double* dF_dm, const double* dF_dv, double* dalpha_out, double* dbeta_out,
                              double* dtheta_out);

/* As mi355gp_vargauss_backward, with the derivative of the bound in K: d var_i / dK = T[:, i] T[:, i]^T (T_kl = Ai_kl beta_k / beta_l),
 * so the dF_dv term of dL_dK is T diag(dF_dv) T^T.  The reference forms np.dot(tmp * dF_dv, tmp.T) with dF_dv a column (:65), which
 * scales the ROWS of tmp; the two agree only where dF_dv is the same at every point (a Gaussian likelihood), and the reference's
 * kernel gradients fail a finite-difference check elsewhere.  dalpha_out and dbeta_out are the same as mi355gp_vargauss_backward's. */
int mi355gp_vargauss_backward_exact(mi355gp_ctx* ctx, const double* dF_dm, const double* dF_dv, double* dalpha_out,
                                    double* dbeta_out, double* dtheta_out);

#ifdef __cplusplus
}
#endif
#endif
