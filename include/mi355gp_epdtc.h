/* mi355gp_epdtc.h -- EPDTC on the sparse context (csrc/epdtc.hip): expectation propagation for a Bernoulli likelihood with
 * the probit link over the DTC posterior q(f) = N(mu, Sigma), Sigma = Knm (Kmm + Kmn diag(tau) Knm)^-1 Kmn, mu = Sigma v
 * (GPy/inference/latent_function_inference/expectation_propagation.py:145-185, 436-578).  A header of its own next to
 * include/mi355gp.h; bound in gpy_amd/_lib.py by the table EPDTC_ABI, which tests/test_oracle_epdtc.py holds against the
 * prototypes here.  All four calls work on a context that mi355gp_sparse_set_data has given X (N x D) and ONE output column
 * (the labels; only their shape is read), that is not row-sharded and holds no input variances.  A positive return value is a
 * LAPACK-style info (the first non-positive pivot), a negative one an error (mi355gp_last_error).
 *
 * The order of a fit: begin (new kernel parameters or Z), then recompute and sweep in any order and number, then inference.
 * Between begin and the last sweep no other call may run on the context: recompute leaves P = LLT^-1 and gamma = P Kmn v
 * behind, and sweep continues from them. */
#ifndef MI355GP_EPDTC_H
#define MI355GP_EPDTC_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The part list, Z (M x D) and Kmm = K(Z) + jitter I; Kmm is factored here so that a matrix that is not positive definite
 * comes back as info before any site is touched (the caller then adds jitter, as jitchol does). */
int mi355gp_epdtc_begin(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M, double jitter);

/* posteriorParamsDTC._recompute (:174-185): LLT = Kmm + sum_n tau_n k_n k_n^T, its factor, P = LLT^-1, gamma = P Kmn v, and
 * for every row mu_n = k_n^T gamma, Sigma_diag_n = |L^-1 k_n|^2 (both N).  tau must be finite and not negative.
 * ms_out (optional): stream time of the call. */
int mi355gp_epdtc_recompute(mi355gp_sparse* s, const double* tau, const double* v, double* mu_out, double* sigdiag_out,
                            double* ms_out);

/* One sequential pass over the sites (:548-575 with parallel_updates = False) in blocks of 64 sites of `order` (a
 * permutation of 0 .. N-1), continuing from the P and gamma of the last recompute.  ysign: +1 / -1 per row.  first != 0: the
 * first site visited sees Sigma_ii + 1e-8 (:538, :547).  tau and v (N) are read and overwritten; the cavity parameters and
 * log Z_hat, mu_hat, sigma2_hat of every site come back as mi355gp_ep_sweep returns them.  Two calls with the same inputs
 * after the same recompute give the same bytes. */
int mi355gp_epdtc_sweep(mi355gp_sparse* s, const int64_t* order, const double* ysign, double eta, double delta, int first,
                        double* tau, double* v, double* cav_tau_out, double* cav_v_out, double* logZhat_out,
                        double* mu_hat_out, double* sigma2_hat_out, double* ms_out);

/* The VarDTC evaluation of the converged sites (:484-492): targets v / tau, per-point precision tau (every entry positive and
 * finite), jitter the whole term on Kmm's diagonal (the reference passes Lm, so var_dtc.py:93 adds nothing).  Two N-vectors
 * are uploaded, not X.  Outputs as mi355gp_vardtc_inference_sum's; dLdR_out (N): the per-point dL_dR.  The result lies where
 * VarDTC's does: mi355gp_sparse_predict, mi355gp_sparse_fetch and mi355gp_sparse_fetch_dLdKnm serve it.  The context's
 * targets are v / tau afterwards. */
int mi355gp_epdtc_inference(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                            const double* tau, const double* v, double jitter, double* out_scalars, double* dtheta_out,
                            double* dZ_out, double* wv_out, double* dLdR_out, double* stage_ms);

#ifdef __cplusplus
}
#endif
#endif
