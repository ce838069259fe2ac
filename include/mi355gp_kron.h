/* mi355gp_kron.h -- exact Gaussian GP regression with inputs on a full Cartesian grid G_1 x ... x G_D (csrc/kron.hip;
 * GPy/inference/latent_function_inference/gaussian_grid_inference.py:35-114, GPy/core/gp_grid.py:87-116, after Gilboa, Saatci and
 * Cunningham 2015): K = K_1 (x) ... (x) K_D, so every quantity is a chain of tensor mode products on N-vectors, N = prod G_d.
 * A header of its own next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table KRON_ABI, which tests/test_oracle_kron.py
 * holds against the prototypes here.  (The mi355gp_grid_* names of mi355gp.h are the block-cyclic multi-GPU mode, another matter.)
 *
 * A context holds y, alpha and two work vectors of N doubles each and nothing larger; the per-dimension matrices (sum G_d^2
 * doubles) come from the host, which builds K_d and takes its eigendecomposition K_d = Q_d diag(lam_d) Q_d^T.  The flat index of
 * an N-vector has the LAST dimension fastest.  A negative return value is an error (mi355gp_last_error).  Every sum is a
 * two-stage fixed-order partial sum and every mode product accumulates k in ascending order: two contexts give the same bytes. */
#ifndef MI355GP_KRON_H
#define MI355GP_KRON_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355gp_kron mi355gp_kron;

#define MI355GP_KRON_MAX_D 16        /* dimensions of the grid */
#define MI355GP_KRON_MAX_G 8192      /* points per dimension */
#define MI355GP_KRON_FETCH_ALPHA 0

int mi355gp_kron_create(int device, mi355gp_kron** out);
int mi355gp_kron_destroy(mi355gp_kron* ctx);

/* The grid sizes G[0..D-1] (each 1 .. MI355GP_KRON_MAX_G, D 1 .. MI355GP_KRON_MAX_D) and the N = prod G_d targets y. */
int mi355gp_kron_set_data(mi355gp_kron* ctx, int D, const int64_t* G, const double* y);

/* Q: the D matrices Q_d (G_d x G_d, row-major, eigenvectors in columns) concatenated; lam: the D eigenvalue vectors concatenated;
 * noise: the whole term on the diagonal (the caller passes sigma^2 + 1e-8).  alpha = (x)Q_d [ (x)Q_d^T y / (V + noise) ] with
 * V_i = prod_d lam_d[i_d] stays resident;  scalars[0] = y^T alpha,  scalars[1] = sum_i log(V_i + noise). */
int mi355gp_kron_solve(mi355gp_kron* ctx, const double* Q, const double* lam, double noise, double* scalars);

/* After solve.  factors: nmat sets of D matrices A_d (G_d x G_d, row-major, concatenated as Q is); gammas: nmat sets of D vectors
 * (concatenated as lam is).  out[2 t] = alpha^T ((x)_d A_d^(t)) alpha,  out[2 t + 1] = sum_i prod_d gamma_d^(t)[i_d] / (V_i + noise). */
int mi355gp_kron_quadforms(mi355gp_kron* ctx, int nmat, const double* factors, const double* gammas, double* out);

/* After solve.  kx: for d = 0..D-1 the M x G_d block K_d(x*_m, grid_d), row-major, concatenated over d; bx: the same layout,
 * bx[d] = kx[d] Q_d.  mu[m] = sum_i alpha_i prod_d kx_d[m][i_d];  var_reduction[m] = sum_i prod_d bx_d[m][i_d]^2 / (V_i + noise_pred).
 * var_reduction (and bx) may be NULL. */
int mi355gp_kron_predict(mi355gp_kron* ctx, int64_t M, const double* kx, const double* bx, double noise_pred, double* mu,
                         double* var_reduction);

/* which = MI355GP_KRON_FETCH_ALPHA: the N doubles of alpha of the last solve */
int mi355gp_kron_fetch(mi355gp_kron* ctx, int which, double* out);

/* One mode product alone, on a context's stream (no data needed): x is P x G row-major, A is R x G row-major (transA = 0) or
 * G x R row-major read transposed (transA = 1);  out[r][p] = sum_k A[r][k] x[p][k], R x P row-major.  reps > 1 repeats the
 * launch; ms_out (may be NULL) receives the HIP-event time of one launch, the mean over the repeats. */
int mi355gp_kron_mode_probe(mi355gp_kron* ctx, int64_t P, int64_t G, int64_t R, int transA, const double* A, const double* x,
                            double* out, int reps, double* ms_out);

/* HIP-event time (ms) of the stream work of the last solve + quadforms pair (solve starts the clock, quadforms adds to it) */
int mi355gp_kron_get_ms(mi355gp_kron* ctx, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif
