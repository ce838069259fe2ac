/* mi355gp_psi_lin.h -- Linear and Bias psi-statistics on the sparse context (csrc/psi_lin.hip, k_grad_rows_lin in
 * csrc/kern_sparse.hip): uncertain-input VarDTC and prediction for ONE input-dependent part, RBF or Linear, summed with Bias and
 * White parts (GPy/kern/src/psi_comp/linear_psi_comp.py, static.py:133-189, the Bias cross terms of add.py:147-266).  A header of
 * its own next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table PSI_LIN_ABI, which tests/test_psi_lin_host.py holds
 * against the prototype here.  The stand-alone probe of the row kernel is a diagnostic: include/mi355gp_debug_psi_lin.h. */
#ifndef MI355GP_PSI_LIN_H
#define MI355GP_PSI_LIN_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: mi355gp_vardtc_inference_uncertain and mi355gp_sparse_predict_uncertain of this context take, with unchanged
 * signatures, one RBF or one Linear part plus any number of Bias and White parts (all summands, one noise variance), and the
 * context's Linear switch (mi355gp_sparse_set_linear) is turned on as well, so that prediction at certain points takes the
 * Linear part.  A new context has it off and refuses Bias and Linear parts under uncertain inputs by name, as every context
 * did before: a caller has to ask.  on == 0 turns this switch off and leaves the Linear switch as it is.  Refused either way:
 * two input-dependent parts (RBF + Linear, two RBFs), products, every other kind, per-point noise, a row-sharded context. */
int mi355gp_sparse_set_psi_lin_bias(mi355gp_sparse* s, int on);

#ifdef __cplusplus
}
#endif
#endif
