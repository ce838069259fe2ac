// psi_ss.h -- launchers of the spike-and-slab psi-statistics kernels (psi_ss.hip) shared by the stateless entry points and the
// spike-and-slab fit of the sparse context (sparse.hip).  Host code only; see psi_ss.hip for the formulas and the buffer
// layouts.  The launch geometry, the split rules and the psi2 combine are psi.h's.
#pragma once
#include "psi.h"

#define PSS_NZ 3               // per-inducing-point sums of a gradient kernel: Zs, Zk, Zq
#define PSS_RL(Qp) (1 + 4 * (Qp))   // doubles of one row record of a gradient kernel: P0, R0[q], R1[q], R2[q], K0[q]

// Ep (mpad x Qp) = exp(-a_q z^2 / 2) over the zero-padded Z
void launch_pss_e(hipStream_t st, const double* Zp, const double* a, long mpad, int Qp, double* Ep);
// per row: rd1 / rd2 (rows x Qp x 4 doubles = (mu, c1 / c2, the slab prefactor, 1 - gamma)); a: Qp entries 1 / l_q^2 (0: not seen)
void launch_pss_rows(hipStream_t st, const double* mu, const double* S, const double* gam, const double* a, long rows, int D,
                     int Qp, double* rd1, double* rd2);
// psi1 rows < rows, columns < m into out (ld ldo); Zp, Ep: mpad x Qp, mpad % 64 == 0
void launch_pss_psi1(hipStream_t st, const double* rd1, const double* Zp, const double* Ep, long rows, long m, long mpad, int Qp,
                     double var, double* out, long ldo);
// part: nsplit x ld x ld (lower 16-tiles), ld >= round_up(m, 16); returns the number of splits written (launch_psi2_combine)
int launch_pss_psi2(hipStream_t st, const double* rd2, const double* w, const double* Zp, const double* Ep, const double* ap,
                    long rows, long m, int Qp, double var2, long ld, double* part);
// Ppart: ceil(m / 16) x rows x PSS_RL(Qp); Zpart: ceil(rows / PSI_GROWS) x mpad x PSS_NZ Qp.  G == NULL: the weights are rk's product
void launch_pss_psi1_grad(hipStream_t st, const double* rd1, const double* Zp, const double* Ep, const double* G, long ldg,
                          PsiRank rk, long rows, long m, long mpad, int Qp, double var, double* Ppart, double* Zpart);
void launch_pss_psi2_grad(hipStream_t st, const double* rd2, const double* w, const double* Zp, const double* Ep,
                          const double* ap, const double* dL, long ldd, long rows, long m, long mpad, int Qp, double var2,
                          double* Ppart, double* Zpart);
// dmu, dS, dgam (rows x D) and rowrec (rows x (1 + Qp)) from the summed row records of psi1 / psi2 (either may be NULL)
void launch_pss_rowfinish(hipStream_t st, const double* P1s, const double* P2s, const double* S, const double* gam, const double* a,
                          long rows, int D, int Qp, double* dmu, double* dS, double* dgam, double* rowrec);
// host: dZ (m x D, optional) += the psi1 and psi2 shares; lsum[q] += the inducing points' share of l_q dE/dl_q.  zs1 / zs2: the
// summed Zpart of psi1 / psi2 (zeros where a statistic was not asked for); zp: Z zero padded to Qp columns
void pss_finish_z(const double* zs1, const double* zs2, const double* a, const double* zp, long m, int D, int Qp, double* dZ,
                  double* lsum);
