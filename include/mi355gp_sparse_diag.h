/* mi355gp_sparse_diag.h -- the per-point diagonal of a kernel expression on the sparse context (csrc/kern_diag.hip): what the
 * sparse inference families share once Kdiag is no longer one number (a Linear part, GPy/kern/src/linear.py:84-85,100-105;
 * sums and products as add.py:74-79, prod.py:67-71,101-111).  A header of its own next to include/mi355gp.h; bound in
 * gpy_amd/_lib.py by the table SPARSE_DIAG_ABI, which tests/test_sparse_lin_host.py holds against the prototypes here. */
#ifndef MI355GP_SPARSE_DIAG_H
#define MI355GP_SPARSE_DIAG_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Linear (kind 9) on this context: on != 0 makes mi355gp_vardtc_inference_sum, mi355gp_pep_inference, mi355gp_svgp_forward /
 * _predict, the mi355gp_epdtc_* calls and mi355gp_sparse_predict take Linear parts -- alone, as summands and as factors of a
 * product with stationary / Bias / Linear factors -- with Kdiag by point.  A new context has it off and refuses kind 9 by name,
 * as every context did before the kind was taken: a caller has to ask.  Still refused either way: a row-sharded context,
 * uncertain inputs, the single-kind entry mi355gp_vardtc_inference. */
int mi355gp_sparse_set_linear(mi355gp_sparse* s, int on);

/* Kdiag of the expression `parts` (the sparse path's kinds, Linear included whatever the switch above says) at the N rows of X that mi355gp_sparse_set_data gave the context:
 *   kd_n = sum over terms of the product of the factors' diagonals at x_n  (White counts with its variance).
 * kd_out (N, optional) receives it.  With weights w (N; NULL: none) the sums a host caller of update_gradients_diag needs:
 *   sums_out[0] = sum_n w_n kd_n,  sums_out[1] = sum_n w_n^2 kd_n,
 *   ddiag_out (the parts' parameters concatenated, in theta order): the gradient of sum_n w_n kd_n -- the variance of a
 *   constant-diagonal part gets sum_n w_n (the other factors' diagonals at x_n), a lengthscale 0, a Linear part
 *   sum_n w_n (the other factors) x_nq^2 per active dimension (their sum for one shared variance).
 * sums_out and ddiag_out are optional and read only when w is given.  Block partial sums are combined in a fixed order, no
 * floating-point atomics: two calls give the same bytes.  The expression is parsed into a list of the call's own: the context's
 * part list, its last inference result and everything mi355gp_sparse_fetch, _fetch_dLdKnm, _predict and an SVGP backward call
 * derive from them stay as they were.  Refused on a row-sharded context. */
int mi355gp_sparse_kdiag(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* w, double* kd_out,
                         double* sums_out, double* ddiag_out);

#ifdef __cplusplus
}
#endif
#endif
