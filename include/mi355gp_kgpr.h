/* mi355gp_kgpr.h -- exact Gaussian GP regression on matrix-shaped data Y (N1 x N2) with the covariance K2(X2) (x) K1(X1) + sigma^2 I of
 * two ARBITRARY kernels (csrc/kgpr.hip; GPy/models/gp_kronecker_gaussian_regression.py, after Stegle et al. 2011).  A header of its
 * own next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table KGPR_ABI, which tests/test_kgpr_host.py holds against the
 * prototypes here.  (The mi355gp_kron_* names are the grid path -- one RBF on a Cartesian grid --, another matter.)
 *
 * The kernels enter as matrices, as with mi355gp_inference_given_K: the caller builds K1 (N1 x N1) and K2 (N2 x N2) and receives
 * dL_dK1 and dL_dK2.  One evaluation decomposes both on the device (csrc/eigh.hip), K_d = U_d diag(S_d) U_d^T, and works with the
 * factors only; nothing of size N1 N2 x N1 N2 exists.  With W[i, j] = S1[i] S2[j] + sigma^2 and Y_ = U1^T Y U2:
 *   Wi = 1 / W,  Ytilde = Y_ o Wi                                     (resident, with U1, S1, U2, S2, until the next evaluation)
 *   lml = -1/2 N1 N2 log 2 pi - 1/2 sum log W - 1/2 sum Y_ o Ytilde,   dL_dsigma2 = -1/2 sum Wi + 1/2 sum Ytilde^2
 *   dL_dK1 = 1/2 T1 diag(S2) T1^T - 1/2 U1 diag(r1) U1^T,  T1 = U1 Ytilde,    r1[i] = sum_j Wi[i, j] S2[j]
 *   dL_dK2 = 1/2 T2 diag(S1) T2^T - 1/2 U2 diag(r2) U2^T,  T2 = U2 Ytilde^T,  r2[j] = sum_i Wi[i, j] S1[i]
 * All matrices are row-major.  A negative return value is an error (mi355gp_last_error).  Every reduction is a fixed-order sum of
 * partials in memory and there are no floating-point atomics: two contexts give the same bytes.
 *
 * Device memory of a context, in doubles, with P_d = N_d rounded up to 128 and L_d = N_d rounded up to MI355GP_EIGH_B:
 *   2 L1^2 + 2 L2^2 + 1100 (L1 + L2)  (the eigensolver's work matrices, partial Grams and rotations)
 *   + P1^2 + P2^2  (U1, U2)  +  max(P1, P2)^2  (K in, dL_dK out)
 *   + 5 P1 P2  (Y, Y_, Ytilde, Wi and one work matrix)  +  (P1 / 32 + 2) P2 + (P2 / 256 + 2) P1  (the marginals' partial sums);
 * set_data refuses by name, before anything is allocated, when that is more than the device has free. */
#ifndef MI355GP_KGPR_H
#define MI355GP_KGPR_H
#include "mi355gp.h"
#include "mi355gp_eigh.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355gp_kgpr mi355gp_kgpr;

#define MI355GP_KGPR_FETCH_U1 0      /* N1 x N1, eigenvectors in columns */
#define MI355GP_KGPR_FETCH_S1 1      /* N1, ascending */
#define MI355GP_KGPR_FETCH_U2 2      /* N2 x N2 */
#define MI355GP_KGPR_FETCH_S2 3      /* N2 */
#define MI355GP_KGPR_FETCH_YTILDE 4  /* N1 x N2 */
#define MI355GP_KGPR_FETCH_WI 5      /* N1 x N2 */
#define MI355GP_KGPR_NUM_MS 9

int mi355gp_kgpr_create(int device, mi355gp_kgpr** out);
int mi355gp_kgpr_destroy(mi355gp_kgpr* ctx);

/* Y: N1 x N2, every entry finite; N1, N2 in 1 .. MI355GP_EIGH_MAX_N.  Allocates everything an evaluation needs. */
int mi355gp_kgpr_set_data(mi355gp_kgpr* ctx, const double* Y, int64_t N1, int64_t N2);

/* K1 (N1 x N1), K2 (N2 x N2): symmetric positive semi-definite (the contract of mi355gp_eigh.h); noise = sigma^2 > 0.
 * scalars[0] = lml, scalars[1] = dL_dsigma2; dL_dK1 (N1 x N1) and dL_dK2 (N2 x N2) are exactly symmetric; sweeps[0..1] (may be NULL)
 * the sweep counts of the two decompositions.  Errors that name themselves: a decomposition that reaches MI355GP_EIGH_MAX_SWEEPS
 * (-3; the factor is named), a W[i, j] <= 0 or not finite (-4: an eigenvalue at -tiny under a very small noise). */
int mi355gp_kgpr_inference(mi355gp_kgpr* ctx, const double* K1, const double* K2, double noise, double* scalars, double* dL_dK1,
                           double* dL_dK2, int* sweeps);

/* After inference.  k1xf: M1 x N1 = K1(X1new, X1); k2xf: M2 x N2; k1xx (M1), k2xx (M2): the diagonals at the new points.  All
 * M1 M2 combinations, flat index i + M1 j:  A = k1xf U1, B = k2xf U2,  mu = (A Ytilde B^T)[i, j],
 * var = k1xx[i] k2xx[j] - ((A o A) Wi (B o B)^T)[i, j] + sigma^2. */
int mi355gp_kgpr_predict(mi355gp_kgpr* ctx, const double* k1xf, int64_t M1, const double* k2xf, int64_t M2, const double* k1xx,
                         const double* k2xx, double* mu, double* var);

/* which = MI355GP_KGPR_FETCH_*: a result of the last inference */
int mi355gp_kgpr_fetch(mi355gp_kgpr* ctx, int which, double* out);

/* HIP-event times (ms) of the last inference: [0] the two decompositions, [1] the four rotations (GEMMs), [2] the spectral pass with
 * its finishing launches, [3] the two weighted-SYRK launches, [4] transfers, [5] all of it, [6] and [7] the weighted SYRK of dL_dK1 and
 * of dL_dK2 alone; [8] the device work of the last predict, transfers included.  MI355GP_KGPR_NUM_MS doubles. */
int mi355gp_kgpr_get_ms(mi355gp_kgpr* ctx, double* ms_out);

/* The weighted symmetric rank-k kernel alone, stateless:  C (n x n) = 1/2 sum_k da[k] Pa[i, k] Pa[j, k] + 1/2 sum_k db[k] Pb[i, k] Pb[j, k]
 * with Pa n x ka, Pb n x kb and signed weights; n in 1 .. MI355GP_EIGH_MAX_N, ka, kb in 1 .. 2 MI355GP_EIGH_MAX_N.  Panel a is summed
 * before panel b, k ascending within slabs of 16; C is exactly symmetric.  reps > 1 repeats the launch; ms (may be NULL): the
 * HIP-event time of one launch, the mean over the repeats. */
int mi355gp_kgpr_wsyrk(int device, int64_t n, const double* Pa, int64_t ka, const double* da, const double* Pb, int64_t kb,
                       const double* db, double* C, int reps, double* ms);

#ifdef __cplusplus
}
#endif
#endif
