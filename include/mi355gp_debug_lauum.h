/* mi355gp_debug_lauum.h -- diagnostic entry points of libmi355gp.so for X^T X on the 128 x 256 tile (csrc/gemm_tile.h, k_lauum_wide),
 * used by tests/ and tools/ only.  Like mi355gp_debug.h, NOT part of the drop-in boundary (include/mi355gp.h); bound in
 * gpy_amd/_lib.py by the table DEBUG_LAUUM_ABI, which tests/test_lauum_wide_map.py holds against the prototypes here. */
#ifndef MI355GP_DEBUG_LAUUM_H
#define MI355GP_DEBUG_LAUUM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Host only (no GPU call): the work list of X^T X on 128 x 256 tiles (k_lauum_wide, csrc/lauum_policy.h) for an nt x nt tile matrix, in
 * launch order.  items: up to max_items rows of 4 ints (tile row ti, first column block tj, column blocks 2 or 1, K in rows);
 * out4 = number of items, 1 if the policy gives a single whole-K launch of this nt the wide tile, the policy's threshold in tiles,
 * number of two-block items.  Returns 0, or -1 if max_items is too small (out4 still set). */
int mi355gp_dbg_lauum_wide_map(int nt, int* items, int max_items, int* out4);
/* Diagnostics: W = X^T X of a lower-triangular n x n matrix (row-major, n a multiple of 128; only tiles on and below the diagonal are
 * read) as ONE whole-K launch on the 128 x 128 tile (variant 0) or the 128 x 256 tile (variant 1), and the average milliseconds of
 * `reps` further launches (reps = 0: none).  X == NULL: a synthetic matrix made on the device; W == NULL: nothing is copied back.
 * W gets the blocks on and below the diagonal; the rest is zero.
 * Variant 2: the product's own choice instead -- lauum_device with a default workspace (k_lauum64 up to 8 tiles per dimension, then
 * the split work list, k_lauum, k_lauum_wide by size).  W is then copied to the device BEFORE the launch as well: blocks above the
 * diagonal, which no X^T X kernel may write, come back as they went in (tests/test_gpu_tileops.py). */
int mi355gp_dbg_lauum(int device, int64_t n, const double* X, double* W, int variant, int reps, double* ms);

#ifdef __cplusplus
}
#endif
#endif
