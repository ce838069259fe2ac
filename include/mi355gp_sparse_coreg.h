/* mi355gp_sparse_coreg.h -- Coregionalize (kind 8, GPy/kern/src/coregionalize.py:82-157) on the sparse context: the switch that
 * makes VarDTC with certain inputs take the multi-output kernels that util.multioutput.ICM / LCM build, with inducing inputs that
 * carry an output index (GPy/models/sparse_gp_coregionalized_regression.py).  A header of its own next to include/mi355gp.h; bound
 * in gpy_amd/_lib.py by the table SPARSE_COREG_ABI, which tests/test_sparse_coreg_host.py holds against the prototype here. */
#ifndef MI355GP_SPARSE_COREG_H
#define MI355GP_SPARSE_COREG_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Coregionalize (kind 8) on this context: on != 0 makes mi355gp_vardtc_inference_sum, mi355gp_sparse_predict and
 * mi355gp_sparse_kdiag take Coregionalize parts -- as factors of a product with stationary / Bias / Linear factors (Linear where
 * mi355gp_sparse_set_linear is on as well) or as a summand -- with Kdiag by point, diag(B) at the row's output.  A part is
 * {kind 8, ard = P <= 16, n_active = 1, active_dims = {the input column of the output index}, theta = B (P x P row-major)};
 * its gradient in dtheta_out is S (P x P): S[a][b] = the sum of dL_dKnm over rows of output a and inducing points of output b,
 * plus the same sum of dL_dKmm over the whole M x M matrix (rows a, columns b), plus on the diagonal the per-output sums of
 * dL_dKdiag.  dZ_out is exactly 0 in the index column.
 *
 * Call it before mi355gp_sparse_set_data: while it is on, set_data keeps the rows on the host, and every call checks the index
 * column its Coregionalize parts name -- of X once per column and P, of Z every time, of new points at prediction -- before
 * anything is launched; the error names the row.  A new context has it off and refuses kind 8 by name, as every context did
 * before.  Still refused either way: a row-sharded context, uncertain inputs, mi355gp_pep_inference, the mi355gp_svgp_* and
 * mi355gp_epdtc_* calls, more than 16 outputs, a White factor inside a product. */
int mi355gp_sparse_set_coregionalize(mi355gp_sparse* s, int on);

#ifdef __cplusplus
}
#endif
#endif
