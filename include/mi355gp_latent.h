/* mi355gp_latent.h -- the exact-GP evaluation with the inputs as parameters (csrc/latent.hip, csrc/exact.hip; GPy/models/gplvm.py):
 * dL/dX = kern.gradients_X(dL_dK, X) comes out of the gradient phase of the evaluation itself, from one pass over the resident
 * Ky^-1 and alpha that also gives the kernel-parameter sums; no N x N array leaves the device or is written.  A header of its own
 * next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table LATENT_ABI, which tests/test_latent_host.py holds against the
 * prototypes here.  A negative return value is an error (mi355gp_last_error). */
#ifndef MI355GP_LATENT_H
#define MI355GP_LATENT_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Re-uploads the inputs of a context after mi355gp_set_data: X is N x D doubles, row-major.  Nothing is reallocated; R, Dy and
 * the options stay. */
int mi355gp_latent_set_X(mi355gp_ctx* ctx, const double* X);

/* mi355gp_exact_inference_sum with the latent-input pass as its gradient phase: the same arguments with the same meaning (the
 * factorisation region is the same code: out_scalars and alpha_out are the same bytes), and dX_out (N x D, row-major) =
 * dL/dX summed over the parts in part order.  Parts: RBF, Matern52, Matern32, Exponential and RatQuad (one launch each); White
 * and Bias add exactly 0.  D <= 32.  Refused by name before any device work: every other kind, product terms (a non-zero term
 * id shared by two parts), D > 32, a context with a Laplace session open. */
int mi355gp_latent_inference_sum(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, const double* noise, int64_t noise_len,
                                 double jitter, double extra_jitter, double* out_scalars, double* alpha_out, double* dtheta_out,
                                 double* dX_out, double* stage_ms);

#ifdef __cplusplus
}
#endif
#endif
