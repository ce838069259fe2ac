/* mi355gp_eigh.h -- fp64 eigendecomposition of a symmetric POSITIVE SEMI-DEFINITE matrix on the device (csrc/eigh.hip): blocked
 * one-sided Jacobi (Hestenes) in column blocks of MI355GP_EIGH_B, the block pairs of one round of a round-robin tournament in one
 * launch.  A header of its own next to include/mi355gp.h; bound in gpy_amd/_lib.py by the table EIGH_ABI, which
 * tests/test_eigh_host.py holds against the prototype here.
 *
 * The contract: A is symmetric and positive semi-definite up to rounding -- every covariance matrix this library builds, the
 * numerically rank-deficient ones included.  An INDEFINITE matrix is outside it and is not served: the method diagonalises A^2,
 * whose eigenvectors are eigenvectors of A only where +lambda and -lambda cannot meet, and nothing here detects the input.  Only
 * the triangle of A with column <= row is read. */
#ifndef MI355GP_EIGH_H
#define MI355GP_EIGH_H
#include "mi355gp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MI355GP_EIGH_B 32            /* columns of a block; a subproblem is 2 B x 2 B */
#define MI355GP_EIGH_MAX_SWEEPS 30   /* the host's sweep loop stops here (measured: 3 to 7 at n <= 163, 11 to 12 at n = 512 .. 4096) */
#define MI355GP_EIGH_MAX_N 16384     /* two padded n x n work matrices, A and V: 8.6 GB there */

/* A: n x n on the host, row-major.  w (n): the eigenvalues in ascending order, each v_j^T (A v_j) with the sign rounding gave it.
 * V (n x n, row-major): the eigenvectors in columns, orthonormal, A V = V diag(w) to working precision.  sweeps (may be NULL): the
 * sweeps that ran, the one that found nothing to rotate included.  ms (may be NULL): HIP-event time of the device work.
 * Returns 0, or 1 when MI355GP_EIGH_MAX_SWEEPS sweeps did not converge (w and V are what the last sweep left), or a negative
 * error (mi355gp_last_error).  Every reduction has a fixed order and there are no floating-point atomics: two calls on the same
 * matrix give the same bytes. */
int mi355gp_eigh(int device, const double* A, int64_t n, double* w, double* V, int* sweeps, double* ms);

#ifdef __cplusplus
}
#endif
#endif
