/* mi355gp_debug_tileops.h -- diagnostic entry point of libmi355gp.so that runs ONE launcher of the fp64 tile-GEMM family
 * (csrc/gemm.hip) alone, on operands the caller supplies, used by tests/ only.  Like mi355gp_debug.h, NOT part of the drop-in
 * boundary (include/mi355gp.h); bound in gpy_amd/_lib.py by the table DEBUG_TILEOPS_ABI, which tests/test_oracle_tileops.py holds
 * against the prototype here.  (The general GEMM has mi355gp_dbg_gemm, X^T X mi355gp_dbg_lauum.) */
#ifndef MI355GP_DEBUG_TILEOPS_H
#define MI355GP_DEBUG_TILEOPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* `op` of mi355gp_dbg_tileop and what `dims` holds for it.  All matrices row-major, every dimension a multiple of 128 except
 * where said; n = 128 nt, m = 128 ntc (or 128 ntother).  Leading dimensions are the ones the product passes: the row length.
 *   TRMM_LOWER    dims = {nt, ntc}                 Out (n x m) = X B      X (n x n) lower triangular, B (n x m)
 *   TRMM_LOWER_T  dims = {nt, ntc}                 Out (n x m) = X^T B
 *   TRMM64        dims = {nt, ntother, mode}       mode 0: Out = alpha X B, 1: alpha X^T B       (B, Out: n x m)
 *                                                  mode 2: Out = alpha B X^T, 3: alpha B X       (B, Out: m x n)
 *   GRAM_SPLITK   dims = {rows, mp, S, accumulate} X = the panel P (rows x mp, rows % (16 S) == 0); Out = S partial matrices
 *                                                  (mp x mp each, in and out): part[s] (+)= P_s^T P_s on the lower tiles; B unused
 *   UPDATE_NT     dims = {K, ntr, ntc, row0t, col0t}   the trailing update inside ONE square matrix, as the blocked Cholesky lays
 *                                                  it out: Out (in and out) is N x N, N = K + 128 max(row0t + ntr, col0t + ntc); its
 *                                                  first K columns are the panel P; the region C of ntr x ntc tiles starts at tile
 *                                                  (K / 128 + row0t, K / 128 + col0t); C -= P[rows of C] P[rows at C's columns]^T on
 *                                                  the tiles on or below the matrix diagonal.  X, B unused.
 * Only tiles of X on or below the diagonal are read.  Out is copied to the device BEFORE the launch (so what a launcher must
 * not write comes back as it went in) and back after it. */
#define MI355GP_TILEOP_TRMM_LOWER 0
#define MI355GP_TILEOP_TRMM_LOWER_T 1
#define MI355GP_TILEOP_TRMM64 2
#define MI355GP_TILEOP_GRAM_SPLITK 3
#define MI355GP_TILEOP_UPDATE_NT 4
int mi355gp_dbg_tileop(int device, int op, const int64_t* dims, const double* X, const double* B, double* Out, double alpha);

#ifdef __cplusplus
}
#endif
#endif
