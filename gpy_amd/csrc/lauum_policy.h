// lauum_policy.h -- which X^T X launches run on the 128 x 256 tile (k_lauum_wide, gemm.hip), and the work list of such a launch.
// Plain C++ without a device call: the kernel, the launcher and the host map entry (mi355gp_dbg_lauum_wide_map,
// tests/test_lauum_wide_map.py) all read the list from here.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define LAUUM_POLICY_HD __host__ __device__
#else
#define LAUUM_POLICY_HD
#endif

// Tiles per dimension from which the single whole-K launch takes the wide tile.  Below nt = 45 X^T X belongs to the 64 x 64
// quadrants and the split work list anyway.  A wide launch has half as many items, each owning a CU for twice as long, so a small
// matrix pays for the better k-loop with a longer ragged end (nt = 48: 600 items on 256 CUs, the first of them 384 slabs long).
// Measured alone (profiles/lauum_wide_ab.txt): N = 6144 slower (1.24 -> 1.35 ms), 7168 and 8192 equal, 9216 ahead (3.93 -> 3.89),
// from 10240 on ahead by 0.7 % growing to 3.8 % at 20480.
#define LAUUM_WIDE_MIN_NT 72

static inline bool lauum_wide_applies(int nt, int force_old) { return !force_old && nt >= LAUUM_WIDE_MIN_NT; }

// Work item b of a wide launch: tile row ti, first column block tj, `wide` = 1 for the pair {tj, tj + 1} (a 128 x 256 tile),
// 0 for a lone block (a 128 x 128 tile: the diagonal block of an even ti, which has no partner at or below the diagonal).
// Both halves of a pair lie in one tile row, so K = (nt - ti) * 128 is uniform inside an item.  Row ti has ti / 2 + 1 items:
// the pairs {0,1}, {2,3}, ... with 2j + 1 <= ti, then (ti even) the diagonal block.  Rows come in ascending ti = longest K first;
// rows 2m and 2m + 1 have m + 1 items each, so m (m + 1) items come before row 2m.
LAUUM_POLICY_HD static inline long lauum_wide_items(int nt) {
    const long m = nt / 2;
    return (nt & 1) ? (m + 1) * (m + 1) : m * (m + 1);
}

LAUUM_POLICY_HD static inline void lauum_wide_item(long b, int& ti, int& tj, int& wide) {
    long m = (long)((sqrtf(4.0f * (float)b + 1.0f) - 1.0f) * 0.5f);
    while (m * (m + 1) > b) --m;
    while ((m + 1) * (m + 2) <= b) ++m;
    long r = b - m * (m + 1);
    ti = (int)(2 * m);
    if (r > m) {
        r -= m + 1;
        ++ti;
    }
    tj = (int)(2 * r);
    wide = (tj + 1 <= ti) ? 1 : 0;
}
