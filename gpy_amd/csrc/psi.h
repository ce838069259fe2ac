// psi.h -- launchers of the psi-statistics kernels (psi.hip) shared by the stateless entry points and the uncertain-input
// fit of the sparse context (sparse.hip).  Host code only; see psi.hip for the formulas and the buffer layouts.
#pragma once
#include "internal.h"

#define PSI_KT 64              // psi1: 64 x 64 output tiles
#define PSI_KDC 32             // dimensions staged in LDS at a time; width of one accumulator group of the gradient kernels
#define PSI_QMAX 64            // most input dimensions the psi kernels take (their LDS staging is sized for it)
#define PSI_T2 16              // psi2: 16 x 16 output tiles, one element per thread
#define PSI_SPLIT_MAX 16       // most row splits of the psi2 sum
#define PSI_GROWS 256          // rows one workgroup of a gradient kernel walks (16 at a time)
#define PSI_CHUNK 2048         // rows per chunk (bounds every partial buffer); psi2 is compute-bound, not HBM-bound
#define PSI_CG 4               // output columns one register group of the psi2n contraction carries
#define PSI_CONTRACT_RB(QP) ((QP) > 32 ? 16 : ((QP) > 16 ? 32 : 64))     // rows a workgroup of the contraction stages (16 KB)
#define PSI_CONTRACT_SPLIT_MAX 64    // most splits of the contraction's lower-tile list
#define PSI_MMAX 65535         // most inducing points: the M x M helper kernels put M in gridDim.y

// dL_dpsi1[n][m] = beta sum_d R[n][d] v[m][d] formed on the fly (the fit's rank-Dy product, var_dtc.py:219)
struct PsiRank {
    const double* R;           // rows x Dy (the chunk's rows)
    const double* v;           // m x Dy
    int Dy;
    double beta;
};

int psi_qp(int D);             // dimensions padded to a power of two up to 32, then to 64
int psi2_nsplit(long rows, long m);
// per row: rd1 / rd2 (rows x Qp double2 = (mu, c1) / (mu, c2)) and lg1 / lg2 (rows); a: Qp entries 1 / l_q^2 (0: not seen)
void launch_psi_rows(hipStream_t st, const double* mu, const double* S, const double* a, long rows, int D, int Qp, double* rd1,
                     double* rd2, double* lg1, double* lg2);
// psi1 rows < rows, columns < m into out (ld ldo); Zp: mpad x Qp zero padded, mpad % 64 == 0
void launch_psi1(hipStream_t st, const double* rd1, const double* lg1, const double* Zp, long rows, long m, long mpad, int Qp,
                 double var, double* out, long ldo);
// part: nsplit x ld x ld (lower 16-tiles), ld >= round_up(m, 16); returns the number of splits written
int launch_psi2(hipStream_t st, const double* rd2, const double* lg2, const double* w, const double* Zp, const double* ap,
                long rows, long m, int Qp, double var2, long ld, double* part);
// out[i][j] (+)= sum_k part[k][max(i,j)][min(i,j)], i, j < m: the fixed-order combine of the splits and the mirror
void launch_psi2_combine(hipStream_t st, const double* part, long ld, long m, int nsplit, int accumulate, double* out, long ldo);
// Ppart: ceil(m / 16) x rows x (1 + 2 Qp); Zpart: ceil(rows / PSI_GROWS) x mpad x Qp.  G == NULL: the weights are rk's product
void launch_psi1_grad(hipStream_t st, const double* rd1, const double* lg1, const double* Zp, const double* G, long ldg,
                      PsiRank rk, long rows, long m, long mpad, int Qp, double var, double* Ppart, double* Zpart);
void launch_psi2_grad(hipStream_t st, const double* rd2, const double* lg2, const double* w, const double* Zp, const double* ap,
                      const double* dL, long ldd, long rows, long m, long mpad, int Qp, double var2, double* Ppart,
                      double* Zpart);
// dmu, dS (rows x D) and rowrec (rows x (1 + Qp)) from the summed P of psi1 / psi2 (either may be NULL)
void launch_psi_rowfinish(hipStream_t st, const double* P1s, const double* P2s, const double* S, const double* a, long rows,
                          int D, int Qp, double* dmu, double* dS, double* rowrec);
// zz (m x 2 Qp): the z_m - z_o sums of dL * psi2 (both ld ldm, dL symmetric)
void launch_psi2_zz(hipStream_t st, const double* dL, const double* psi2, long ldm, const double* Zp, long m, int Qp, double* zz);
// Prediction at uncertain points: part[split][n][c] (splits x rows x (Dy + 1)) = the split's share of
// sum_mo psi2n[m][o] lam[m][c] lam[o][c] (c < Dy; lam: m x Dy) and of sum_mo psi2n[m][o] W[m][o] (c == Dy; W ld ldw); returns the
// number of splits written, psi_contract_nsplit(rows, m, Qp) (sum them with launch_sum_splits: a fixed order)
int psi_contract_nsplit(long rows, long m, int Qp);
int launch_psi2n_contract(hipStream_t st, const double* rd2, const double* lg2, const double* Zp, const double* ap,
                          const double* lam, int Dy, const double* W, long ldw, long rows, long m, int Qp, double var2,
                          double* part);
// var (rows x Dy) = max(psi0 + C[n][d] - C[n][Dy] - mean[n][d]^2, 1e-15); C: rows x (Dy + 1)
void launch_psi_predvar(hipStream_t st, const double* C, const double* mean, double psi0, long rows, int Dy, double* var);
