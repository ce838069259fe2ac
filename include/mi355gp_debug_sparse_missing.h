/* mi355gp_debug_sparse_missing.h -- diagnostics of the group-batched psi2 kernels (csrc/psi_missing.hip): the stateless pair of
 * include/mi355gp_sparse_missing.h with a switch for the route the batched kernels replace and the stream time of the psi2 kernels,
 * for tools/missing_time.py and the A/B tests.  Bound in gpy_amd/_lib.py by the table DEBUG_MISSING_ABI, which
 * tests/test_oracle_missing.py holds against the prototypes here.  No product code calls these. */
#ifndef MI355GP_DEBUG_SPARSE_MISSING_H
#define MI355GP_DEBUG_SPARSE_MISSING_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mi355gp_rbf_psi2_groups.  loop != 0: the single-mask kernel of mi355gp_rbf_psi once per group with weights W[:, g] (the same sums
 * in the same order).  ms_out (optional): the stream time of the psi2 kernels alone, HIP events around the launches, summed over
 * the row chunks. */
int mi355gp_dbg_rbf_psi2_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                                const double* mu, const double* S, int64_t N, int D, const double* W, int G, int loop,
                                double* psi2_out, double* ms_out);

/* mi355gp_rbf_psi_grad_groups with the same two extras (ms_out: the psi2 gradient kernels alone). */
int mi355gp_dbg_rbf_psi_grad_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                                    const double* mu, const double* S, int64_t N, int D, const double* W, int G,
                                    const double* dL_dpsi2, int loop, double* dvar_out, double* dl_out, double* dZ_out,
                                    double* dmu_out, double* dS_out, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif
