// eigh.h -- the on-device form of the symmetric PSD eigensolver (eigh.hip) for callers inside the library.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

// Everything one decomposition of an n x n matrix needs on the device, sized once by eigh_ws_alloc and reusable for any call of
// the same n: G and V column-major L x L (L = n rounded up to the block width), the per-pair partial Grams and rotations.
struct EighWs {
    DevBuf G, V, part, J, norm2, lam, tiny2;
    DevArr<int> pair_rot, flags, rank;
    long n = 0, L = 0;
    int nb = 0, T = 0, chr = 0, nch = 0;
};
int eigh_ws_alloc(EighWs* ws, long n);

// A (device, n x n with row stride lda, symmetric PSD; its triangle with column <= row is read) -> w (device, n, ascending) and
// V (device, n x n with row stride ldv, eigenvectors in columns).  The launches go to `st`; the host waits for the stream once per
// sweep to read the sweep's flag.  Returns 0, 1 (the sweep cap was reached) or a negative error; *sweeps (optional) the count.
int eigh_device(hipStream_t st, const double* A, long lda, long n, double* w, double* V, long ldv, EighWs* ws, int* sweeps);
