// psi_missing.h -- launchers of the group-batched psi2 kernels (psi_missing.hip): psi2 and its chain rule for several row
// masks at once.  Output columns of Y that share a set of observed rows form a group g with row weights w_g; a launch takes up to
// PSI_GB groups and evaluates every exponential once for all of them.  Host code; see psi_missing.hip for the layouts.
#pragma once
#include "internal.h"
#include "psi.h"

#define PSI_GB 8               // groups one launch of a multi kernel carries (accumulators / staged dL matrices per thread block)

// inducing points o the multi gradient kernel stages at a time: its dL tiles are PSI_GB times those of k_psi2_grad
inline int psi_multi_oc(int Qp) { return Qp > 32 ? 8 : 16; }

// wt: the weights GROUP-major, wt[g * ldw + n] for the batch's groups g < gb <= PSI_GB and the chunk's rows n < rows.
// part: gb x nsplit x ld x ld (lower 16-tiles), ld >= round_up(m, 16); returns nsplit = psi2_nsplit(rows, m): group g's partial
// sums start at part + g * nsplit * ld * ld (finish each with launch_psi2_combine)
int launch_psi2_multi(hipStream_t st, const double* rd2, const double* lg2, const double* wt, long ldw, int gb, const double* Zp,
                      const double* ap, long rows, long m, int Qp, double var2, long ld, double* part);
// The row pass of the psi2 chain rule with the per-row weight sum_g w_ng dL_g[m][o]: dL = gb symmetric matrices (ld ldd),
// group g's at dL + g * dstride.  Ppart / Zpart as launch_psi2_grad.
void launch_psi2_grad_multi(hipStream_t st, const double* rd2, const double* lg2, const double* wt, long ldw, int gb,
                            const double* Zp, const double* ap, const double* dL, long dstride, long ldd, long rows, long m,
                            long mpad, int Qp, double var2, double* Ppart, double* Zpart);
