/* mi355gp_sparse_missing.h -- the psi2 side of a Bayesian GPLVM with missing data: psi2 of the RBF kernel and its chain rule for
 * several row masks at once (csrc/psi_missing.hip; GPy/models/sparse_gp_minibatch.py:228-286).  Output columns of Y that share a
 * set of observed rows form a group g with row weights W[:, g]; a kernel launch carries up to mi355gp_psi_groups_batch() groups
 * and evaluates every exponential once for all of them.  A header of its own next to include/mi355gp.h; bound in gpy_amd/_lib.py
 * by the table MISSING_ABI, which tests/test_oracle_missing.py holds against the prototypes here.  The first three calls are stateless: they
 * upload, compute and download.  Every sum is combined in a fixed order (groups, chunks, splits ascending; no floating-point
 * atomics): two calls with the same arguments give the same bytes, and every psi2_g is bitwise symmetric. */
#ifndef MI355GP_SPARSE_MISSING_H
#define MI355GP_SPARSE_MISSING_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The number of groups one launch of a group-batched kernel carries (a compile-time constant of the library). */
int mi355gp_psi_groups_batch(void);

/* psi2_g = sum_n W[n][g] psi2n for g < G into psi2_out (G x M x M).  lengthscale: D entries if ard, else one.  Z: M x D; mu, S:
 * N x D, S positive; W: N x G row-major, every entry finite (a bad entry is refused with its row and column).  D > 64 is refused
 * by name. */
int mi355gp_rbf_psi2_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                            const double* mu, const double* S, int64_t N, int D, const double* W, int G, double* psi2_out);

/* The five gradients of sum_g sum(sym(dL_dpsi2_g) * psi2_g) (rbf_psi_comp.py:70-133 with a per-row dL_dpsi2[n] = sum_g W[n][g]
 * dL_dpsi2_g): dL_dpsi2 is G x M x M (each matrix symmetrised inside).  dl_out: D entries if ard, else one; dZ_out M x D; dmu_out,
 * dS_out N x D.  A row with weight 0 in every group gets exactly 0 in dmu_out and dS_out. */
int mi355gp_rbf_psi_grad_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                                const double* mu, const double* S, int64_t N, int D, const double* W, int G,
                                const double* dL_dpsi2, double* dvar_out, double* dl_out, double* dZ_out, double* dmu_out,
                                double* dS_out);

/* ---- the sparse context (mi355gp_sparse_create ... of mi355gp.h) with missing entries of Y ---------------------------------- */

/* The row masks of Y's columns: G groups, group_of_output (Dy ints, the group of every output column) and W (N x G row-major,
 * 0 / 1: row n is observed by group g).  Valid after set_data and mi355gp_sparse_set_input_variance (missing data is handled on
 * the uncertain-input path).  Y must already hold 0 where unobserved: an entry that is not finite, or not 0 where its group does
 * not observe it, is refused by row and column.  A group with no observed row is refused with its first output.  G = 0 clears
 * the groups.  mi355gp_sparse_set_data forgets them; mi355gp_sparse_set_inputs keeps them (a GPLVM step uploads 2 N Q doubles).
 * Refused by name: a context without input variances, with slab probabilities, asked for psi_lin_bias / linear / coregionalize,
 * or row-sharded. */
int mi355gp_sparse_set_output_groups(mi355gp_sparse* s, int G, const int* group_of_output, const double* W);

/* One VarDTC evaluation with missing data: mi355gp_vardtc_inference_uncertain's parameters.  One RBF part alone or with White
 * parts, one noise variance.  out_scalars is the sum over the groups (a per-group copy: mi355gp_sparse_fetch_group_scalars);
 * wv_out (M x Dy) holds every group's Woodbury columns in their output positions; dmu_out / dS_out are exactly 0 on a row no
 * output observes.  Refused by name before any device work: a context without groups, per-point noise, every kind but RBF and
 * White.  (mi355gp_vardtc_inference_uncertain and mi355gp_vardtc_inference_ss in turn refuse a context WITH groups.)  Afterwards
 * the context's current woodbury_inv and psi2 are group 0's. */
int mi355gp_vardtc_inference_missing(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                     const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars,
                                     double* dtheta_out, double* dZ_out, double* wv_out, double* dmu_out, double* dS_out,
                                     double* stage_ms);

/* Makes group g's woodbury_inv and psi2 the context's current ones, so that mi355gp_sparse_predict,
 * mi355gp_sparse_predict_uncertain and mi355gp_sparse_fetch serve the outputs of that group (the per-output variance of
 * posterior.py:243-246, :268; the mean comes from all Dy Woodbury columns in any one call). */
int mi355gp_sparse_select_output_group(mi355gp_sparse* s, int g);

/* The per-group copies of out_scalars of the last mi355gp_vardtc_inference_missing call: G x 8, rows in group order. */
int mi355gp_sparse_fetch_group_scalars(mi355gp_sparse* s, double* out);

#ifdef __cplusplus
}
#endif
#endif
