// psi.h -- launchers of the psi-statistics kernels (psi.hip) shared by the stateless entry points and the uncertain-input
// fit of the sparse context (sparse.hip).  Host code but for psi_tile and the two reductions that end a gradient workgroup; see psi.hip for the formulas and the buffer layouts.
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

// lower 16 x 16 tile number -> (ti, tj), ti >= tj (device; shared by the psi2 kernels of psi.hip and psi_ss.hip)
__device__ __forceinline__ void psi_tile(long tl, int* ti, int* tj) {
    long i = (long)((sqrt(8.0 * (double)tl + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > tl) --i;
    while ((i + 1) * (i + 2) / 2 <= tl) ++i;
    *ti = (int)i;
    *tj = (int)(tl - i * (i + 1) / 2);
}

// ---- the two reductions that end a workgroup of a gradient kernel (device; psi.hip and psi_missing.hip) -------------------
// Ppart[mtile][row][1 + 2 Qp]: P0, P1[q], P2[q] summed over the tile's 16 inducing points (lane shuffles, fixed tree)
template <int QG>
__device__ __forceinline__ void psi_grad_emit(int t, int gz, int Qp, long n, bool nvalid, double a0, double* g1, double* g2,
                                              double* __restrict__ prow) {
    // sum over the 16 lanes that share a row; lane ml == 0 stores
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
        a0 += __shfl_xor(a0, s);
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            g1[q] += __shfl_xor(g1[q], s);
            g2[q] += __shfl_xor(g2[q], s);
        }
    }
    if ((t & 15) == 0 && nvalid) {
        if (gz == 0) prow[0] = a0;
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            prow[1 + gz * PSI_KDC + q] = g1[q];
            prow[1 + Qp + gz * PSI_KDC + q] = g2[q];
        }
    }
}

// sum zacc over the 16 rows of the workgroup (4 per wave by shuffles, 4 waves through LDS in wave order) and store
template <int QG>
__device__ __forceinline__ void psi_grad_emit_z(int t, int gz, int Qp, long mcol, long mpad, double* zacc, double* zred,
                                                double* __restrict__ zblock) {
#pragma unroll
    for (int q = 0; q < QG; ++q) {
        zacc[q] += __shfl_xor(zacc[q], 16);
        zacc[q] += __shfl_xor(zacc[q], 32);
    }
    const int lane = t & 63, wv = t >> 6;
    if (lane < 16)
#pragma unroll
        for (int q = 0; q < QG; ++q) zred[(wv * 16 + lane) * QG + q] = zacc[q];
    __syncthreads();
    if (t < 16 && mcol < mpad)
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const double s = (zred[(0 * 16 + t) * QG + q] + zred[(1 * 16 + t) * QG + q]) +
                             (zred[(2 * 16 + t) * QG + q] + zred[(3 * 16 + t) * QG + q]);
            zblock[mcol * Qp + gz * PSI_KDC + q] = s;
        }
}

// dL_dpsi1[n][m] = beta sum_d R[n][d] v[m][d] formed on the fly (the fit's rank-Dy product, var_dtc.py:219)
struct PsiRank {
    const double* R;           // rows x Dy (the chunk's rows)
    const double* v;           // m x Dy
    int Dy;
    double beta;
};

// ... plus add[m] on every row (the Bias parts' share of dL_dpsi1: b t^T, t = 2 rowsum(dL_dpsi2)); a kernel instantiated for
// PsiRank itself is the code it was before this form existed
struct PsiRankAdd : PsiRank {
    const double* add;         // m
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
                      PsiRank rk, long rows, long m, long mpad, int Qp, double var, double* Ppart, double* Zpart,
                      const double* add = nullptr);     // add (m, optional, with G == NULL only): see PsiRankAdd
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
// ---- psi_lin.hip: the M-sized helpers of a Linear part and of Bias parts under uncertain inputs -----------
// psi2[i][j] += sum_q (il_q^4 sums[q]) Z[i][q] Z[j][q], i, j < m (Z: m x D row-major, il / sums: device)
void launch_psi2_rank_add(hipStream_t st, const double* Z, const double* il, const double* sums, long m, int D, double* psi2, long ld);
// out (m x D) = A Z for a symmetric A (leading m x m of ld)
void launch_mm_times_z(hipStream_t st, const double* A, long ld, const double* Z, long m, int D, double* out);
// out[j] = scale sum_{i < m} A[i][j]
void launch_mm_colsums(hipStream_t st, const double* A, long ld, long m, double scale, double* out);
// psi2[i][j] += b (c[i] + c[j]) + nb2;  psi1Y[j][d] += b vs[d]   (i, j < m)
void launch_psi2_bias_add(hipStream_t st, double* psi2, long ld, long m, const double* c, double b, double nb2);
void launch_psi1y_bias_add(hipStream_t st, double* psi1Y, long m, int Dy, const double* vs, double b);
// var[n][d] = max(base[n] + sum_q S[n][q] g[d][q], 1e-15)   (S: rows x D, g: Dy x D)
void launch_lin_predvar(hipStream_t st, const double* base, const double* S, const double* g, long rows, int D, int Dy, double* var);
// mean[n][d] += bsl[d];  C (optional, rows x (Dy + 1)): C[n][d] += sum_j psi1[n][j] u[j][d] + cst[d]
void launch_psi_bias_pred(hipStream_t st, const double* psi1, long ldp, const double* u, const double* cst, const double* bsl, long rows,
                          long m, int Dy, double* C, double* mean);
// var (rows x Dy) = max(psi0 + C[n][d] - C[n][Dy] - mean[n][d]^2, 1e-15); C: rows x (Dy + 1)
void launch_psi_predvar(hipStream_t st, const double* C, const double* mean, double psi0, long rows, int Dy, double* var);
