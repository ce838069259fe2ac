/* mi355gp_debug_psi_lin.h -- diagnostics of the Linear psi-statistics (csrc/psi_lin.hip): the row kernel k_grad_rows_lin on its own,
 * for tests/test_gpu_psi_lin.py and tools/psi_lin_time.py.  No part of the drop-in boundary; bound in gpy_amd/_lib.py by the
 * table DEBUG_PSI_LIN_ABI, which tests/test_psi_lin_host.py holds against the prototype here. */
#ifndef MI355GP_DEBUG_PSI_LIN_H
#define MI355GP_DEBUG_PSI_LIN_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The row-side kernel of a Linear part on its own, for tests and timing:
 *   out[i][q] = variances_q sum_j g[i][j] Z[j][q] + c0 variances_q X[i][q]                      (rows x D)
 * with the weights g[i][j] = W[i][j] (rows x M) when Y is NULL, otherwise rowscale_i (gscale W[i][j] + beta sum_d Y[i][d] V[j][d])
 * (Y: rows x Dy, V: M x Dy, rowscale: rows or NULL = 1) formed on the fly.  fused != 0: the MFMA kernel (D <= 16); 0: the weights
 * in memory, then the plain kernel (D <= 64).  X and Z are scaled by sqrt(variances) as the sparse context scales them.
 * ms_out (optional, reps doubles) with reps >= 1: after the launch that gives `out`, the kernel is launched reps more times, each
 * between two HIP events of its own on the launching stream; ms_out[k] = the time of launch k in milliseconds (the fused kernel
 * alone; fused == 0: the plain kernel without the formation of the weights).  The caller discards warm-ups and takes a median. */
int mi355gp_dbg_psi_lin_rows(int device, int fused, const double* W, const double* Y, const double* V, const double* rowscale,
                               double beta, double gscale, const double* X, const double* Z, const double* variances, double c0,
                               int64_t rows, int64_t M, int D, int Dy, double* out, int reps, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif
