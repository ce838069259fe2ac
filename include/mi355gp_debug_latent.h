/* mi355gp_debug_latent.h -- diagnostic of the latent-input gradient pass (csrc/latent.hip): the kernel k_latent_grad with its two
 * finishing launches on its own, for tests/test_gpu_latent.py and tools/latent_time.py.  No part of the drop-in boundary; bound in
 * gpy_amd/_lib.py by the table DEBUG_LATENT_ABI, which tests/test_latent_host.py holds against the prototype here. */
#ifndef MI355GP_DEBUG_LATENT_H
#define MI355GP_DEBUG_LATENT_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One stationary part (kind 0-3 or 6, theta in the kind's order) over all D <= 32 columns of X (N x D).  W: ANY symmetric N x N
 * matrix in the place of Ky^-1, alpha: N x Dy -- the kernel is judged free of the conditioning of a factorisation.  With
 * g_ij = 0.5 (alpha_i . alpha_j - Dy W_ij) and h_ij = g_ij (dK/dr) / r (0 where r = 0):
 *   dX_out[i][q] = (2 / l_q) sum_j h_ij (x_iq - x_jq) / l_q                                     (N x D)
 *   rec_out[0] = sum g K, [1] = sum h r^2 (isotropic), [2 + q] = sum h ((x_iq - x_jq) / l_q)^2 (ARD),
 *   rec_out[34] = sum g dK/dpower (RatQuad)                                                     (68 doubles, the rest 0) */
int mi355gp_dbg_latent_grad(int device, int kind, int ard, const double* theta, const double* X, int64_t N, int D, const double* W,
                            const double* alpha, int Dy, double* dX_out, double* rec_out);

#ifdef __cplusplus
}
#endif
#endif
