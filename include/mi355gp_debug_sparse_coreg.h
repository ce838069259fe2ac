/* mi355gp_debug_sparse_coreg.h -- a diagnostic of the sparse context for tests and tools, next to include/mi355gp_debug.h: the
 * A/B switch between the gradient passes that are fused with their column reductions and the routes they replace.  Bound in
 * gpy_amd/_lib.py by the table DEBUG_SPARSE_COREG_ABI, which tests/test_sparse_coreg_host.py holds against the prototype here. */
#ifndef MI355GP_DEBUG_SPARSE_COREG_H
#define MI355GP_DEBUG_SPARSE_COREG_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* on == 0: this context's second pass takes the unfused routes -- the generic gradient kernel with H written and a column
 * reduction for a stationary part, the weights formed in memory for a Linear part, and for a stationary x Coregionalize term the
 * product route (the other factor's K-build, dL_dKnm multiplied up in memory, each factor's own kernel) in place of
 * k_grad_cols_icm.  on != 0 (a new context): the fused passes wherever they apply.  Both compute the same quantities; the bytes
 * differ, as the order of the sums does. */
int mi355gp_dbg_sparse_set_fuse_cols(mi355gp_sparse* s, int on);

#ifdef __cplusplus
}
#endif
#endif
