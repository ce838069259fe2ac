// grad_policy.h -- which launch of the exact path's gradient pass runs as k_grad_tilegemm (kern.hip).  Plain C++ without a
// device call, so that a host test can compile it on its own (tests/test_grad_policy.py).
#pragma once
#include <stdint.h>

#include "../../include/mi355gp.h"

struct GradLaunchCase {
    int fused;              // dL_dK formed on the fly from Ky^-1 and alpha (the exact path), not read from G
    int kind, ard;
    int has_mul;            // factor of a product kernel: dL_dK times the other factors' covariances
    int has_hout;           // the weights of the gradients_X reductions go out
    int has_rank;           // the sparse path's rank term
    uintptr_t w_addr;       // Ky^-1 and its leading dimension: a thread row of four weights is ONE 32-byte load
    long ldw;
    int force_old;          // the A/B switch of the diagnostics build
};

// The tile-GEMM form serves the fused ARD pass of RBF, Matern-5/2 and Matern-3/2 on the padded, 32-byte aligned Ky^-1 of the
// exact context; everything else takes k_grad and keeps its bits.  The Exponential kernel stays there too: the division of its
// dK/dr / r takes the instantiation past the 168 VGPRs of three waves per SIMD (105 spilled), which is what the form is for.
static inline bool grad_tilegemm_applies(const GradLaunchCase& c) {
    if (c.force_old || !c.fused || !c.ard) return false;
    if (c.kind != MI355GP_RBF && c.kind != MI355GP_MATERN52 && c.kind != MI355GP_MATERN32) return false;
    if (c.has_mul || c.has_hout || c.has_rank) return false;
    return (c.w_addr & 31u) == 0 && c.ldw % 4 == 0;
}
