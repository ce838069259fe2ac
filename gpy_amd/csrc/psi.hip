// psi.hip -- psi-statistics of the RBF kernel for Gaussian inputs q(x_n) = N(mu_n, diag S_n), and their gradients.
// Restates (does not port) GPy/kern/src/psi_comp/rbf_psi_comp.py:22-50 (psi1, psi2) and :70-133 (the chain rule from
// dL_dpsi0/1/2 to variance, lengthscale, Z, mu, S), one of the two pieces of device code of the reference (rbf_psi_gpucomp.py;
// the other, ssrbf_psi_gpucomp.py for spike-and-slab inputs, has its counterpart in psi_ss.hip).
// With a_q = 1 / l_q^2 (0 on a dimension the kernel does not see), c1 = a / (S a + 1), c2 = a / (2 S a + 1):
//   psi1[n,m]  = var   exp(-1/2 sum_q log(S a + 1)  - 1/2 sum_q c1 (mu - z_m)^2)
//   psi2n[m,o] = var^2 exp(-1/2 sum_q log(2 S a + 1) - sum_q a (z_m - z_o)^2 / 4 - sum_q c2 (mu - (z_m + z_o)/2)^2)
// The squared differences are evaluated directly (the expanded form of rbf_psi_comp.py:48 cancels for large |mu|), the same
// choice the covariance build makes for r^2.  psi2n does not factor over (n,m) x (n,o): there is no GEMM here, the work is
// one fp64 exp and a Q-long sum per (n, m, o).
// Every sum over n, m or o is combined in a fixed order (per-workgroup partials, then launch_sum_splits-style passes):
// two evaluations give the same bits; there are no floating-point atomics.
//
// Gradients: with L1 = dL_dpsi1 * psi1 and L2[n] = w_n dL_dpsi2 * psi2n (dL_dpsi2 symmetrised, rbf_psi_comp.py:109), both
// gradient kernels produce per row n and dimension q
//   P0 = sum L, P1 = sum L d, P2 = sum L d^2          (d = mu - z_m, resp. mu - (z_m + z_o)/2; sums over m, resp. m and o)
// and per inducing point m and dimension q   Zs = sum c L d (over n, resp. n and o).  psi2n is recomputed tile by tile, an
// N x M x M array never exists.  k_psi_rowfinish turns the P into dmu, dS and the per-row variance / lengthscale sums; the
// z_m - z_o terms of psi2 need only the M x M matrix dL_dpsi2 * psi2 (k_psi2_zz).
//
// Prediction at uncertain points (posterior.py:249-269) contracts psi2n per row against given M x M weights: k_psi2n_contract.
#include <cmath>
#include <type_traits>
#include <vector>

#include "../../include/mi355gp.h"
#include "internal.h"
#include "parts.h"
#include "psi.h"

#define PSI_OC 32              // inducing points o staged at a time by the psi2 gradient kernel (61 KB of LDS at 64 dimensions)

int psi_qp(int D) {     // dimensions padded to a power of two up to 32, then to 64; the padding has a = 0, mu = z = 0
    int q = 1;
    while (q < D && q < 32) q <<= 1;
    return D <= 32 ? q : PSI_QMAX;
}

// per row: rd1[n][q] = (mu, c1), rd2[n][q] = (mu, c2), lg1[n] = -1/2 sum log(S a + 1), lg2[n] = -1/2 sum log(2 S a + 1)
__global__ void k_psi_rows(const double* __restrict__ mu, const double* __restrict__ S, const double* __restrict__ a, long rows,
                           int D, int Qp, double2* __restrict__ rd1, double2* __restrict__ rd2, double* __restrict__ lg1,
                           double* __restrict__ lg2) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    double s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < Qp; ++q) {
        double2 v1 = make_double2(0.0, 0.0), v2 = v1;
        if (q < D) {
            const double aq = a[q], m = mu[n * D + q], s = S[n * D + q];
            const double d1 = fma(s, aq, 1.0), d2 = fma(2.0 * s, aq, 1.0);
            s1 += log(d1);
            s2 += log(d2);
            v1 = make_double2(m, aq / d1);
            v2 = make_double2(m, aq / d2);
        }
        rd1[n * Qp + q] = v1;
        rd2[n * Qp + q] = v2;
    }
    lg1[n] = -0.5 * s1;
    lg2[n] = -0.5 * s2;
}

// psi1 tile: 64 rows x 64 inducing points, thread = one column and 16 rows, dimensions in groups of PSI_KDC.
// Zp: mpad x Qp (zero padded, mpad % 64 == 0).  Writes rows < rows, columns < m of out (ld ldo).
__global__ __launch_bounds__(256) void k_psi1(const double2* __restrict__ rd, const double* __restrict__ lg1,
                                              const double* __restrict__ Zp, long rows, long m, int Qp, double var,
                                              double* __restrict__ out, long ldo) {
    __shared__ double zs[PSI_KT * (PSI_KDC + 1)];
    __shared__ double2 rs[PSI_KT * PSI_KDC];
    const int t = threadIdx.x, mc = t & 63, g = t >> 6;
    const long n0 = (long)blockIdx.x * PSI_KT, m0 = (long)blockIdx.y * PSI_KT;
    double e[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) e[k] = 0.0;
    for (int qg = 0; qg < Qp; qg += PSI_KDC) {
        const int qn = (Qp - qg < PSI_KDC) ? (Qp - qg) : PSI_KDC;
        for (int idx = t; idx < PSI_KT * qn; idx += 256) {
            const int r = idx / qn, q = idx - r * qn;
            zs[r * (PSI_KDC + 1) + q] = Zp[(m0 + r) * Qp + qg + q];
            rs[r * PSI_KDC + q] = (n0 + r < rows) ? rd[(n0 + r) * Qp + qg + q] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        for (int q = 0; q < qn; ++q) {
            const double z = zs[mc * (PSI_KDC + 1) + q];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const double2 v = rs[(g * 16 + k) * PSI_KDC + q];
                const double d = v.x - z;
                e[k] = fma(v.y * d, d, e[k]);
            }
        }
        __syncthreads();
    }
    if (m0 + mc >= m) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const long n = n0 + g * 16 + k;
        if (n < rows) out[n * ldo + m0 + mc] = var * exp(fma(-0.5, e[k], lg1[n]));
    }
}

// psi2 partial sums: part[split][mi][oj] (ld x ld, lower 16-tiles) = var^2 sum over the split's rows of w_n psi2n[mi][oj] / var^2.
// Thread = one (m, o) with the midpoint (z_m + z_o)/2 in registers; rows come through LDS (every lane reads the same row).
template <int QP>
__global__ __launch_bounds__(256) void k_psi2(const double2* __restrict__ rd2, const double* __restrict__ lg2,
                                              const double* __restrict__ w, const double* __restrict__ Zp,
                                              const double* __restrict__ ap, long rows, long rps, long m, double var2, long ld,
                                              double* __restrict__ part) {
    constexpr int RB = QP > 32 ? 32 : 64;                    // rows staged at a time
    __shared__ double2 rs[RB * QP];
    __shared__ double lgs[RB], ws[RB];
    int ti, tj;
    psi_tile(blockIdx.x, &ti, &tj);
    const int t = threadIdx.x;
    const long mi = (long)ti * PSI_T2 + (t >> 4), oj = (long)tj * PSI_T2 + (t & 15);
    double zb[QP];
    double zd = 0.0;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        const double zm = Zp[mi * QP + q], zo = Zp[oj * QP + q], dz = zm - zo;
        zb[q] = 0.5 * (zm + zo);
        zd = fma(ap[q] * dz, dz, zd);
    }
    zd *= 0.25;
    const long r0 = (long)blockIdx.y * rps, r1 = (r0 + rps < rows) ? (r0 + rps) : rows;
    double acc = 0.0;
    for (long rb = r0; rb < r1; rb += RB) {
        for (int idx = t; idx < RB * QP; idx += 256) {
            const long n = rb + idx / QP;
            rs[idx] = (n < r1) ? rd2[n * QP + (idx % QP)] : make_double2(0.0, 0.0);
        }
        if (t < RB) {
            const long n = rb + t;
            lgs[t] = (n < r1) ? lg2[n] : 0.0;
            ws[t] = (n < r1) ? (w ? w[n] : 1.0) : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < RB; ++r) {
            double e = zd;
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                const double2 v = rs[r * QP + q];
                const double d = v.x - zb[q];
                e = fma(v.y * d, d, e);
            }
            acc = fma(ws[r], exp(lgs[r] - e), acc);
        }
        __syncthreads();
    }
    if (mi < m && oj < m) part[(long)blockIdx.y * ld * ld + mi * ld + oj] = var2 * acc;
}

// out[i][j] (+)= sum_k part[k][max(i,j)][min(i,j)] for i, j < m: the fixed-order combine of the row splits and the mirror
__global__ void k_psi2_combine(const double* __restrict__ part, long ld, long m, int nsplit, int accumulate,
                               double* __restrict__ out, long ldo) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= m) return;
    const long a = (i >= j) ? i : j, b = (i >= j) ? j : i;
    double s = accumulate ? out[i * ldo + j] : 0.0;
    for (int k = 0; k < nsplit; ++k) s += part[(long)k * ld * ld + a * ld + b];
    out[i * ldo + j] = s;
}

// ---- prediction at uncertain points: psi2n contracted per row against given matrices ---------------------------------------
// part[split][n][c] = sum over the split's lower (m, o) tiles of psi2n[m][o] * wgt_c[m][o], c < Dy + 1, with
//   wgt_c = lam[m][c] lam[o][c] for c < Dy (woodbury_vector, M x Dy) and wgt_Dy = W[m][o] (woodbury_inv, ld ldw):
// the two sums of Posterior._raw_predict at uncertain points (posterior.py:262-266); an off-diagonal tile stands for its
// mirror as well (factor 2 on lam lam^T, W[m][o] + W[o][m]).  A workgroup owns RB rows (staged in LDS once) and walks its
// tiles tl = split, split + nsplit, ... in that order.  Per tile and 16 rows: thread (m, o) evaluates psi2n once into LDS
// (Ps, 16 x 256); then thread (row, slice) sums 16 of the 256 values against PSI_CG output columns at a time -- weights
// formed in LDS from the tile's 2 x 16 rows of lam -- the 16 slices are added by lane shuffles (fixed tree) and the slice-0
// lane adds the sum to ITS element of part: one thread, program order, no atomics.  Neither an N* x M x M array nor Dy
// M x M matrices exist.  Static LDS: 16 (rows) + 32 (Ps) + 8 (weights) + 1.5 KB at every QP.
template <int QP>
__global__ __launch_bounds__(256) void k_psi2n_contract(const double2* __restrict__ rd2, const double* __restrict__ lg2,
                                                        const double* __restrict__ Zp, const double* __restrict__ ap,
                                                        const double* __restrict__ lam, int Dy, const double* __restrict__ W,
                                                        long ldw, long rows, long m, long ntl, int nsplit, double var2,
                                                        double* __restrict__ part) {
    constexpr int RB = PSI_CONTRACT_RB(QP);
    __shared__ double2 rs[RB * QP];
    __shared__ double lgs[RB];
    __shared__ double Ps[16 * 256];
    __shared__ double wt[PSI_CG * 256];
    __shared__ double lamT[2 * 16 * PSI_CG];
    const int t = threadIdx.x, NC = Dy + 1;
    const long rb0 = (long)blockIdx.y * RB;
    const int nr = (rows - rb0 < RB) ? (int)(rows - rb0) : RB;           // rows of this workgroup (>= 1)
    for (int idx = t; idx < RB * QP; idx += 256) {
        const int r = idx / QP;
        rs[idx] = (r < nr) ? rd2[(rb0 + r) * QP + (idx % QP)] : make_double2(0.0, 0.0);
    }
    if (t < RB) lgs[t] = (t < nr) ? lg2[rb0 + t] : 0.0;
    const int br = t >> 4, ks = t & 15;                                  // the contraction's (row, slice)
    bool first = true;
    for (long tl = blockIdx.x; tl < ntl; tl += nsplit) {
        int ti, tj;
        psi_tile(tl, &ti, &tj);
        const long mi = (long)ti * PSI_T2 + (t >> 4), oj = (long)tj * PSI_T2 + (t & 15);
        const bool ok = mi < m && oj < m;
        double zb[QP];
        double zd = 0.0;
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            const double zm = Zp[mi * QP + q], zo = Zp[oj * QP + q], dz = zm - zo;
            zb[q] = 0.5 * (zm + zo);
            zd = fma(ap[q] * dz, dz, zd);
        }
        zd *= 0.25;
        const double f = (ti == tj) ? 1.0 : 2.0;
        const double wmo = ok ? ((ti == tj) ? W[mi * ldw + oj] : W[mi * ldw + oj] + W[oj * ldw + mi]) : 0.0;
        for (int sb = 0; sb < nr; sb += 16) {
            __syncthreads();                                             // Ps is free (and rs / lgs are stored)
#pragma unroll 4
            for (int r = 0; r < 16; ++r) {
                double e = zd;
#pragma unroll
                for (int q = 0; q < QP; ++q) {
                    const double2 v = rs[(sb + r) * QP + q];
                    const double d = v.x - zb[q];
                    e = fma(v.y * d, d, e);
                }
                Ps[r * 256 + t] = ok ? var2 * exp(lgs[sb + r] - e) : 0.0;
            }
            for (int g0 = 0; g0 < NC; g0 += PSI_CG) {
                if (t < 2 * 16 * PSI_CG) {                               // the tile's rows of lam: [0] m side, [1] o side
                    const int side = t / (16 * PSI_CG), r = (t / PSI_CG) & 15, c = t % PSI_CG;
                    const long row = (side ? (long)tj : (long)ti) * PSI_T2 + r;
                    lamT[t] = (row < m && g0 + c < Dy) ? lam[row * Dy + g0 + c] : 0.0;
                }
                __syncthreads();                                         // (also: Ps complete, the last contraction done)
#pragma unroll
                for (int c = 0; c < PSI_CG; ++c) {
                    const double ll = f * lamT[(t >> 4) * PSI_CG + c] * lamT[(16 + (t & 15)) * PSI_CG + c];
                    wt[c * 256 + t] = (g0 + c < Dy) ? (ok ? ll : 0.0) : (g0 + c == Dy ? wmo : 0.0);
                }
                __syncthreads();
                double acc[PSI_CG];
#pragma unroll
                for (int c = 0; c < PSI_CG; ++c) acc[c] = 0.0;
                for (int j = 0; j < 16; ++j) {
                    const double p = Ps[br * 256 + j * 16 + ks];
#pragma unroll
                    for (int c = 0; c < PSI_CG; ++c) acc[c] = fma(p, wt[c * 256 + j * 16 + ks], acc[c]);
                }
#pragma unroll
                for (int s = 1; s < 16; s <<= 1)
#pragma unroll
                    for (int c = 0; c < PSI_CG; ++c) acc[c] += __shfl_xor(acc[c], s);
                if (ks == 0 && sb + br < nr) {
                    double* o = part + ((long)blockIdx.x * rows + rb0 + sb + br) * NC + g0;
#pragma unroll
                    for (int c = 0; c < PSI_CG; ++c)
                        if (g0 + c < NC) o[c] = first ? acc[c] : o[c] + acc[c];
                }
            }
        }
        first = false;
    }
}

// var[n][d] = max(psi0 + C[n][d] - C[n][Dy] - mean[n][d]^2, 1e-15)   (posterior.py:262-268; C: rows x (Dy + 1))
__global__ void k_psi_predvar(const double* __restrict__ C, const double* __restrict__ mean, double psi0, long rows, int Dy,
                              double* __restrict__ var) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * Dy) return;
    const long n = i / Dy;
    const double mu = mean[i], v = psi0 + C[n * (Dy + 1) + (i - n * Dy)] - C[n * (Dy + 1) + Dy] - mu * mu;
    var[i] = v < 1e-15 ? 1e-15 : v;
}

// ---- gradient kernels --------------------------------------------------------------------------------------------
// Both: workgroup = 16 inducing points (ml = lane & 15) x 16 rows at a time (nl = thread >> 4), PSI_GROWS rows in all;
// blockIdx.z = accumulator group of PSI_KDC dimensions (the exponent always runs over all Qp dimensions).
//   Ppart[mtile][row][1 + 2 Qp]: P0, P1[q], P2[q] summed over the tile's 16 inducing points (lane shuffles, fixed tree)
//   Zpart[rowblock][m][Qp]:      sum over the block's rows (and all o) of c L d
// LDS (dynamic): zm 16 x (Qp + 1) | rows 16 x Qp double2 | (psi2 only) zo PSI_OC x Qp, dLs PSI_OC x 16 | zred 4 x 16 x QG

// (psi_grad_emit / psi_grad_emit_z, the two reductions that end a gradient workgroup, are in psi.h: psi_missing.hip shares them)

// psi1: L = G[n][m] var exp(lg1 - 1/2 sum c1 d^2), d = mu - z_m
// (RK = PsiRankAdd: the rank product plus add[m] per column; RK = PsiRank compiles to the code it always was)
template <int QG, class RK>
__global__ __launch_bounds__(256) void k_psi1_grad(const double2* __restrict__ rd, const double* __restrict__ lg1,
                                                   const double* __restrict__ Zp, const double* __restrict__ G, long ldg,
                                                   RK rk, long rows, long m, long mpad, int Qp, double var,
                                                   double* __restrict__ Ppart, double* __restrict__ Zpart) {
    extern __shared__ __align__(16) double sm[];
    double* zm = sm;                                           // 16 x (Qp + 1)
    double2* rs = (double2*)(sm + 16 * (Qp + 2));              // 16 x Qp   (offset even: 16-byte aligned)
    double* zred = (double*)(rs + 16 * Qp);                    // 4 x 16 x QG
    const int t = threadIdx.x, ml = t & 15, nl = t >> 4, gz = blockIdx.z, qoff = gz * PSI_KDC;
    const long mcol = (long)blockIdx.x * 16 + ml, nb0 = (long)blockIdx.y * PSI_GROWS;
    const int RL = 1 + 2 * Qp;
    for (int idx = t; idx < 16 * Qp; idx += 256) {
        const int r = idx / Qp, q = idx - r * Qp;
        zm[r * (Qp + 1) + q] = Zp[((long)blockIdx.x * 16 + r) * Qp + q];
    }
    double zacc[QG];
#pragma unroll
    for (int q = 0; q < QG; ++q) zacc[q] = 0.0;
    for (int it = 0; it < PSI_GROWS / 16; ++it) {
        const long nbase = nb0 + it * 16;
        if (nbase >= rows) break;                              // (uniform over the workgroup)
        __syncthreads();
        for (int idx = t; idx < 16 * Qp; idx += 256) {
            const long n = nbase + idx / Qp;
            rs[idx] = (n < rows) ? rd[n * Qp + (idx % Qp)] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        const long n = nbase + nl;
        const bool ok = n < rows && mcol < m;
        double e = 0.0;
        for (int q = 0; q < Qp; ++q) {
            const double2 v = rs[nl * Qp + q];
            const double d = v.x - zm[ml * (Qp + 1) + q];
            e = fma(v.y * d, d, e);
        }
        double gw = 0.0;                                       // dL_dpsi1[n][m]: given, or beta R_n . v_m formed here
        if (ok) {
            if (G) gw = G[n * ldg + mcol];
            else {
                for (int d = 0; d < rk.Dy; ++d) gw = fma(rk.R[n * rk.Dy + d], rk.v[mcol * rk.Dy + d], gw);
                gw *= rk.beta;
                if constexpr (std::is_same<RK, PsiRankAdd>::value) gw += rk.add[mcol];
            }
        }
        const double L = ok ? gw * var * exp(fma(-0.5, e, lg1[n])) : 0.0;
        double g1[QG], g2[QG];
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const double2 v = rs[nl * Qp + qoff + q];
            const double d = v.x - zm[ml * (Qp + 1) + qoff + q];
            g1[q] = L * d;
            g2[q] = g1[q] * d;
            zacc[q] = fma(v.y, g1[q], zacc[q]);
        }
        psi_grad_emit<QG>(t, gz, Qp, n, n < rows, L, g1, g2, Ppart + ((long)blockIdx.x * rows + (n < rows ? n : 0)) * RL);
    }
    psi_grad_emit_z<QG>(t, gz, Qp, mcol, mpad, zacc, zred, Zpart + (long)blockIdx.y * mpad * Qp);
}

// psi2: L = w_n dL[m][o] var^2 exp(lg2 - zd[m][o] - sum c2 d^2), d = mu - (z_m + z_o)/2; dL symmetric, read as dL[o][m]
template <int QG>
__global__ __launch_bounds__(256) void k_psi2_grad(const double2* __restrict__ rd, const double* __restrict__ lg2,
                                                   const double* __restrict__ w, const double* __restrict__ Zp,
                                                   const double* __restrict__ ap, const double* __restrict__ dL, long ldd,
                                                   long rows, long m, long mpad, int Qp, double var2,
                                                   double* __restrict__ Ppart, double* __restrict__ Zpart) {
    extern __shared__ __align__(16) double sm[];
    double* zm = sm;                                           // 16 x (Qp + 1)
    double2* rs = (double2*)(sm + 16 * (Qp + 2));              // 16 x Qp
    double* zo = (double*)(rs + 16 * Qp);                      // PSI_OC x Qp
    double* dLs = zo + PSI_OC * Qp;                            // PSI_OC x 16: dL[o][m] var^2 exp(-zd[m][o])
    double* zred = dLs + PSI_OC * 16;                          // 4 x 16 x QG
    const int t = threadIdx.x, ml = t & 15, nl = t >> 4, gz = blockIdx.z, qoff = gz * PSI_KDC;
    const long mcol = (long)blockIdx.x * 16 + ml, nb0 = (long)blockIdx.y * PSI_GROWS;
    const int RL = 1 + 2 * Qp;
    for (int idx = t; idx < 16 * Qp; idx += 256) {
        const int r = idx / Qp, q = idx - r * Qp;
        zm[r * (Qp + 1) + q] = Zp[((long)blockIdx.x * 16 + r) * Qp + q];
    }
    double zacc[QG];
#pragma unroll
    for (int q = 0; q < QG; ++q) zacc[q] = 0.0;
    for (int it = 0; it < PSI_GROWS / 16; ++it) {
        const long nbase = nb0 + it * 16;
        if (nbase >= rows) break;
        __syncthreads();
        for (int idx = t; idx < 16 * Qp; idx += 256) {
            const long n = nbase + idx / Qp;
            rs[idx] = (n < rows) ? rd[n * Qp + (idx % Qp)] : make_double2(0.0, 0.0);
        }
        const long n = nbase + nl;
        const bool nok = n < rows;
        const double wn = nok ? (w ? w[n] : 1.0) : 0.0, lg = nok ? lg2[n] : 0.0;
        double a0 = 0.0, g1[QG], g2[QG];
#pragma unroll
        for (int q = 0; q < QG; ++q) g1[q] = g2[q] = 0.0;
        for (long oc = 0; oc < m; oc += PSI_OC) {
            const int on = (m - oc < PSI_OC) ? (int)(m - oc) : PSI_OC;
            __syncthreads();                                   // (also orders the stores of zm / rs before their first use)
            for (int idx = t; idx < on * Qp; idx += 256) zo[idx] = Zp[oc * Qp + idx];
            __syncthreads();
            for (int idx = t; idx < on * 16; idx += 256) {
                const int o = idx >> 4, c = idx & 15;
                const long mc = (long)blockIdx.x * 16 + c;
                double zd = 0.0;
                for (int q = 0; q < Qp; ++q) {
                    const double dz = zm[c * (Qp + 1) + q] - zo[o * Qp + q];
                    zd = fma(ap[q] * dz, dz, zd);
                }
                dLs[idx] = (mc < m) ? dL[(oc + o) * ldd + mc] * var2 * exp(-0.25 * zd) : 0.0;
            }
            __syncthreads();
            for (int o = 0; o < on; ++o) {
                double e = 0.0;
                for (int q = 0; q < Qp; ++q) {
                    const double2 v = rs[nl * Qp + q];
                    const double d = v.x - 0.5 * (zm[ml * (Qp + 1) + q] + zo[o * Qp + q]);
                    e = fma(v.y * d, d, e);
                }
                const double L = dLs[o * 16 + ml] * wn * exp(lg - e);
                a0 += L;
#pragma unroll
                for (int q = 0; q < QG; ++q) {
                    const double d = rs[nl * Qp + qoff + q].x - 0.5 * (zm[ml * (Qp + 1) + qoff + q] + zo[o * Qp + qoff + q]);
                    const double Ld = L * d;
                    g1[q] += Ld;
                    g2[q] = fma(Ld, d, g2[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < QG; ++q) zacc[q] = fma(rs[nl * Qp + qoff + q].y, g1[q], zacc[q]);
        psi_grad_emit<QG>(t, gz, Qp, n, nok, a0, g1, g2, Ppart + ((long)blockIdx.x * rows + (nok ? n : 0)) * RL);
    }
    __syncthreads();
    psi_grad_emit_z<QG>(t, gz, Qp, mcol, mpad, zacc, zred, Zpart + (long)blockIdx.y * mpad * Qp);
}

// rows of the chunk: dmu, dS (n x D, stored) and rowrec[n][1 + Qp] = {variance sum, lengthscale sums} from the summed P of
// psi1 (P1s) and psi2 (P2s), either may be NULL.  With d1 = S a + 1, d2 = 2 S a + 1:
//   psi1: dmu = -c1 P1, dS = (c1^2 P2 - c1 P0)/2,  l_q dE/dl_q = c1 S P0 + (c1/d1) P2,       variance sum P0
//   psi2: dmu = -2 c2 P1, dS = 2 c2^2 P2 - c2 P0,  l_q dE/dl_q = 2 (c2 S P0 + (c2/d2) P2),   variance sum 2 P0
__global__ void k_psi_rowfinish(const double* __restrict__ P1s, const double* __restrict__ P2s, const double* __restrict__ S,
                                const double* __restrict__ a, long rows, int D, int Qp, double* __restrict__ dmu,
                                double* __restrict__ dS, double* __restrict__ rowrec) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    const int RL = 1 + 2 * Qp;
    const double p01 = P1s ? P1s[n * RL] : 0.0, p02 = P2s ? P2s[n * RL] : 0.0;
    rowrec[n * (1 + Qp)] = p01 + 2.0 * p02;
    for (int q = 0; q < Qp; ++q) {
        double gm = 0.0, gs = 0.0, gl = 0.0;
        if (q < D) {
            const double aq = a[q], s = S[n * D + q];
            if (P1s) {
                const double d1 = fma(s, aq, 1.0), c1 = aq / d1, p1 = P1s[n * RL + 1 + q], p2 = P1s[n * RL + 1 + Qp + q];
                gm -= c1 * p1;
                gs += 0.5 * (c1 * c1 * p2 - c1 * p01);
                gl += c1 * s * p01 + (c1 / d1) * p2;
            }
            if (P2s) {
                const double d2 = fma(2.0 * s, aq, 1.0), c2 = aq / d2, p1 = P2s[n * RL + 1 + q], p2 = P2s[n * RL + 1 + Qp + q];
                gm -= 2.0 * c2 * p1;
                gs += 2.0 * c2 * c2 * p2 - c2 * p02;
                gl += 2.0 * (c2 * s * p02 + (c2 / d2) * p2);
            }
            dmu[n * D + q] = gm;
            dS[n * D + q] = gs;
        }
        rowrec[n * (1 + Qp) + 1 + q] = gl;
    }
}

// the z_m - z_o terms of psi2 from LS = dL_dpsi2 * psi2 (M x M): zz[m][q] = sum_o LS[m][o] (z_mq - z_oq),
// zz[m][Qp + q] = sum_o LS[m][o] (z_mq - z_oq)^2; one workgroup per m, fixed tree
__global__ __launch_bounds__(256) void k_psi2_zz(const double* __restrict__ dL, const double* __restrict__ psi2, long ldm,
                                                 const double* __restrict__ Zp, long m, int Qp, double* __restrict__ zz) {
    __shared__ double r1[256], r2[256];
    const int t = threadIdx.x;
    const long mi = blockIdx.x;
    for (int q = 0; q < Qp; ++q) {
        double s1 = 0.0, s2 = 0.0;
        const double zmq = Zp[mi * Qp + q];
        for (long o = t; o < m; o += 256) {
            const double ls = dL[mi * ldm + o] * psi2[mi * ldm + o], dz = zmq - Zp[o * Qp + q];
            s1 = fma(ls, dz, s1);
            s2 = fma(ls * dz, dz, s2);
        }
        r1[t] = s1;
        r2[t] = s2;
        __syncthreads();
        for (int k = 128; k > 0; k >>= 1) {
            if (t < k) {
                r1[t] += r1[t + k];
                r2[t] += r2[t + k];
            }
            __syncthreads();
        }
        if (t == 0) {
            zz[mi * 2 * Qp + q] = r1[0];
            zz[mi * 2 * Qp + Qp + q] = r2[0];
        }
        __syncthreads();
    }
}

// out = (A + A^T) / 2 over m x m (rbf_psi_comp.py:109)
__global__ void k_psi_symmetrise(const double* __restrict__ A, long m, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j < m) out[i * m + j] = 0.5 * (A[i * m + j] + A[j * m + i]);
}

// ---- launchers -------------------------------------------------------------------------------------------------
int psi2_nsplit(long rows, long m) {
    const long nt = (m + PSI_T2 - 1) / PSI_T2, ntl = nt * (nt + 1) / 2;
    long s = (1024 + ntl - 1) / ntl;                           // about four workgroups per CU
    const long smax = (rows + 63) / 64;
    if (s > smax) s = smax;
    if (s > PSI_SPLIT_MAX) s = PSI_SPLIT_MAX;
    return s < 1 ? 1 : (int)s;
}

template <int QP>
static void launch_psi2_t(hipStream_t st, const double2* rd2, const double* lg2, const double* w, const double* Zp,
                          const double* ap, long rows, long m, double var2, long ld, int nsplit, double* part) {
    const long nt = (m + PSI_T2 - 1) / PSI_T2, ntl = nt * (nt + 1) / 2;
    const long rps = round_up((rows + nsplit - 1) / nsplit, 64);
    hipLaunchKernelGGL((k_psi2<QP>), dim3((unsigned)ntl, (unsigned)nsplit), dim3(256), 0, st, rd2, lg2, w, Zp, ap, rows, rps, m,
                       var2, ld, part);
}
// part: nsplit x ld x ld, ld >= round_up(m, 16); returns the number of splits written (combine with k_psi2_combine)
static int launch_psi2_d2(hipStream_t st, const double2* rd2, const double* lg2, const double* w, const double* Zp,
                       const double* ap, long rows, long m, int Qp, double var2, long ld, double* part) {
    const int ns = psi2_nsplit(rows, m);
    switch (Qp) {
        case 1: launch_psi2_t<1>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 2: launch_psi2_t<2>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 4: launch_psi2_t<4>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 8: launch_psi2_t<8>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 16: launch_psi2_t<16>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 32: launch_psi2_t<32>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
        default: launch_psi2_t<64>(st, rd2, lg2, w, Zp, ap, rows, m, var2, ld, ns, part); break;
    }
    return ns;
}

static size_t psi_grad_lds(int Qp, int QG, bool second) {
    size_t d = 16 * (Qp + 2) + 2 * 16 * Qp + 4 * 16 * QG;
    if (second) d += (size_t)PSI_OC * Qp + PSI_OC * 16;
    return d * sizeof(double);
}
#define PSI_QG_SWITCH(QG, CALL)        \
    switch (QG) {                      \
        case 1: { CALL(1); } break;    \
        case 2: { CALL(2); } break;    \
        case 4: { CALL(4); } break;    \
        case 8: { CALL(8); } break;    \
        case 16: { CALL(16); } break;  \
        default: { CALL(32); } break;  \
    }
// Ppart: ceil(m / 16) x rows x (1 + 2 Qp); Zpart: ceil(rows / PSI_GROWS) x mpad x Qp
void launch_psi1_grad(hipStream_t st, const double* rd1, const double* lg1, const double* Zp, const double* G, long ldg,
                      PsiRank rk, long rows, long m, long mpad, int Qp, double var, double* Ppart, double* Zpart,
                      const double* add) {
    const int QG = Qp < PSI_KDC ? Qp : PSI_KDC;
    const dim3 grid((unsigned)((m + 15) / 16), (unsigned)((rows + PSI_GROWS - 1) / PSI_GROWS), (unsigned)(Qp / QG));
    const size_t lds = psi_grad_lds(Qp, QG, false);
    if (add && !G) {
        const PsiRankAdd rka{rk, add};
#define PSI_CALL(N) hipLaunchKernelGGL((k_psi1_grad<N, PsiRankAdd>), grid, dim3(256), lds, st, (const double2*)rd1, lg1, Zp, G, ldg, rka, rows, m, mpad, Qp, var, Ppart, Zpart)
        PSI_QG_SWITCH(QG, PSI_CALL)
#undef PSI_CALL
        return;
    }
#define PSI_CALL(N) hipLaunchKernelGGL((k_psi1_grad<N, PsiRank>), grid, dim3(256), lds, st, (const double2*)rd1, lg1, Zp, G, ldg, rk, rows, m, mpad, Qp, var, Ppart, Zpart)
    PSI_QG_SWITCH(QG, PSI_CALL)
#undef PSI_CALL
}
void launch_psi2_grad(hipStream_t st, const double* rd2, const double* lg2, const double* w, const double* Zp, const double* ap,
                      const double* dL, long ldd, long rows, long m, long mpad, int Qp, double var2, double* Ppart,
                      double* Zpart) {
    const int QG = Qp < PSI_KDC ? Qp : PSI_KDC;
    const dim3 grid((unsigned)((m + 15) / 16), (unsigned)((rows + PSI_GROWS - 1) / PSI_GROWS), (unsigned)(Qp / QG));
    const size_t lds = psi_grad_lds(Qp, QG, true);
#define PSI_CALL(N) hipLaunchKernelGGL((k_psi2_grad<N>), grid, dim3(256), lds, st, (const double2*)rd2, lg2, w, Zp, ap, dL, ldd, rows, m, mpad, Qp, var2, Ppart, Zpart)
    PSI_QG_SWITCH(QG, PSI_CALL)
#undef PSI_CALL
}

// ---- the launchers psi.h declares -----------------------------------------------------------------------------------
int launch_psi2(hipStream_t st, const double* rd2, const double* lg2, const double* w, const double* Zp, const double* ap,
                long rows, long m, int Qp, double var2, long ld, double* part) {
    return launch_psi2_d2(st, (const double2*)rd2, lg2, w, Zp, ap, rows, m, Qp, var2, ld, part);
}
void launch_psi_rows(hipStream_t st, const double* mu, const double* S, const double* a, long rows, int D, int Qp, double* rd1,
                     double* rd2, double* lg1, double* lg2) {
    hipLaunchKernelGGL(k_psi_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, mu, S, a, rows, D, Qp, (double2*)rd1,
                       (double2*)rd2, lg1, lg2);
}
void launch_psi1(hipStream_t st, const double* rd1, const double* lg1, const double* Zp, long rows, long m, long mpad, int Qp,
                 double var, double* out, long ldo) {
    hipLaunchKernelGGL(k_psi1, dim3((unsigned)((rows + PSI_KT - 1) / PSI_KT), (unsigned)(mpad / PSI_KT)), dim3(256), 0, st,
                       (const double2*)rd1, lg1, Zp, rows, m, Qp, var, out, ldo);
}
void launch_psi2_combine(hipStream_t st, const double* part, long ld, long m, int nsplit, int accumulate, double* out, long ldo) {
    hipLaunchKernelGGL(k_psi2_combine, dim3((unsigned)((m + 255) / 256), (unsigned)m), dim3(256), 0, st, part, ld, m, nsplit,
                       accumulate, out, ldo);
}
void launch_psi_rowfinish(hipStream_t st, const double* P1s, const double* P2s, const double* S, const double* a, long rows,
                          int D, int Qp, double* dmu, double* dS, double* rowrec) {
    hipLaunchKernelGGL(k_psi_rowfinish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, P1s, P2s, S, a, rows, D, Qp, dmu,
                       dS, rowrec);
}
void launch_psi2_zz(hipStream_t st, const double* dL, const double* psi2, long ldm, const double* Zp, long m, int Qp, double* zz) {
    hipLaunchKernelGGL(k_psi2_zz, dim3((unsigned)m), dim3(256), 0, st, dL, psi2, ldm, Zp, m, Qp, zz);
}

int psi_contract_nsplit(long rows, long m, int Qp) {
    const long nt = (m + PSI_T2 - 1) / PSI_T2, ntl = nt * (nt + 1) / 2, rb = PSI_CONTRACT_RB(Qp), nrb = (rows + rb - 1) / rb;
    long s = (1024 + nrb - 1) / nrb;                           // about four workgroups per CU
    if (s > ntl) s = ntl;
    if (s > PSI_CONTRACT_SPLIT_MAX) s = PSI_CONTRACT_SPLIT_MAX;
    return s < 1 ? 1 : (int)s;
}
template <int QP>
static void launch_psi2n_contract_t(hipStream_t st, const double2* rd2, const double* lg2, const double* Zp, const double* ap,
                                    const double* lam, int Dy, const double* W, long ldw, long rows, long m, int ns, double var2,
                                    double* part) {
    const long nt = (m + PSI_T2 - 1) / PSI_T2, ntl = nt * (nt + 1) / 2, nrb = (rows + PSI_CONTRACT_RB(QP) - 1) / PSI_CONTRACT_RB(QP);
    hipLaunchKernelGGL((k_psi2n_contract<QP>), dim3((unsigned)ns, (unsigned)nrb), dim3(256), 0, st, rd2, lg2, Zp, ap, lam, Dy, W,
                       ldw, rows, m, ntl, ns, var2, part);
}
int launch_psi2n_contract(hipStream_t st, const double* rd2, const double* lg2, const double* Zp, const double* ap,
                          const double* lam, int Dy, const double* W, long ldw, long rows, long m, int Qp, double var2,
                          double* part) {
    const int ns = psi_contract_nsplit(rows, m, Qp);
    const double2* rd = (const double2*)rd2;
    switch (Qp) {
        case 1: launch_psi2n_contract_t<1>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
        case 2: launch_psi2n_contract_t<2>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
        case 4: launch_psi2n_contract_t<4>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
        case 8: launch_psi2n_contract_t<8>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
        case 16: launch_psi2n_contract_t<16>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
        case 32: launch_psi2n_contract_t<32>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
        default: launch_psi2n_contract_t<64>(st, rd, lg2, Zp, ap, lam, Dy, W, ldw, rows, m, ns, var2, part); break;
    }
    return ns;
}
void launch_psi_predvar(hipStream_t st, const double* C, const double* mean, double psi0, long rows, int Dy, double* var) {
    hipLaunchKernelGGL(k_psi_predvar, dim3((unsigned)((rows * Dy + 255) / 256)), dim3(256), 0, st, C, mean, psi0, rows, Dy, var);
}

// ---- the stateless entry points ----------------------------------------------------------------------------------
namespace {
// what both entry points validate and upload: the kernel's parameters, Z (padded) and the Gaussian inputs
struct PsiInputs {
    PartSpec spec;
    int D = 0, Qp = 0;
    long N = 0, M = 0, mpad = 0;
    double var = 0.0;
    std::vector<double> a;                                    // Qp: 1 / l_q^2, 0 in the padding
    DevBuf dA, dZp, dMu, dS, dW;
    int load(const char* where, double variance, const double* lengthscale, int ard, const double* Z, int64_t M_,
             const double* mu, const double* S, int64_t N_, int D_, const double* weights) {
        if (!(lengthscale && Z && mu && S && M_ > 0 && N_ > 0 && D_ > 0)) PART_FAIL("%s: bad arguments", where);
        if (M_ > PSI_MMAX) PART_FAIL("%s: %lld inducing points; the psi-statistics kernels take at most %d", where, (long long)M_, PSI_MMAX);
        if (D_ > PSI_QMAX) PART_FAIL("%s: %d input dimensions; the psi-statistics kernels take at most %d", where, D_, PSI_QMAX);
        std::vector<double> th(1 + (size_t)(ard ? D_ : 1));
        th[0] = variance;
        for (size_t k = 1; k < th.size(); ++k) th[k] = lengthscale[k - 1];
        const mi355gp_part part{MI355GP_RBF, ard ? 1 : 0, 0, nullptr, th.data(), 0};
        if (int rc = parse_part(part, D_, 1u << MI355GP_RBF, where, &spec)) return rc;
        for (int64_t i = 0; i < N_ * D_; ++i)
            if (!(S[i] > 0.0) || !std::isfinite(S[i]) || !std::isfinite(mu[i]))
                PART_FAIL("%s: input variance S[%lld][%lld] = %g (mean %g): every entry must be positive and finite", where,
                          (long long)(i / D_), (long long)(i % D_), S[i], mu[i]);
        if (weights)
            for (int64_t i = 0; i < N_; ++i)
                if (!std::isfinite(weights[i])) PART_FAIL("%s: weight %lld is not finite", where, (long long)i);
        D = D_;
        N = N_;
        M = M_;
        Qp = psi_qp(D);
        mpad = round_up(M, PSI_KT);
        var = variance;
        a.assign((size_t)Qp, 0.0);
        for (int q = 0; q < D; ++q) a[(size_t)q] = spec.inv_ls[(size_t)q] * spec.inv_ls[(size_t)q];
        std::vector<double> zp((size_t)mpad * Qp, 0.0);
        for (long i = 0; i < M; ++i)
            for (int q = 0; q < D; ++q) zp[(size_t)i * Qp + q] = Z[i * D + q];
        HIP_CHECK(dA.alloc(Qp));
        HIP_CHECK(dZp.alloc(zp.size()));
        HIP_CHECK(dMu.alloc(N * D));
        HIP_CHECK(dS.alloc(N * D));
        HIP_CHECK(hipMemcpy(dA, a.data(), sizeof(double) * Qp, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dZp, zp.data(), sizeof(double) * zp.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dMu, mu, sizeof(double) * N * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dS, S, sizeof(double) * N * D, hipMemcpyHostToDevice));
        if (weights) {
            HIP_CHECK(dW.alloc(N));
            HIP_CHECK(hipMemcpy(dW, weights, sizeof(double) * N, hipMemcpyHostToDevice));
        }
        return 0;
    }
};
// the per-row operands of one chunk
struct PsiRows {
    DevBuf rd1, rd2, lg1, lg2;
    int alloc(long rows, int Qp) {
        HIP_CHECK(rd1.alloc(2 * rows * Qp));
        HIP_CHECK(rd2.alloc(2 * rows * Qp));
        HIP_CHECK(lg1.alloc(rows));
        HIP_CHECK(lg2.alloc(rows));
        return 0;
    }
    void fill(hipStream_t st, const PsiInputs& in, long r0, long rc) {
        launch_psi_rows(st, in.dMu + r0 * in.D, in.dS + r0 * in.D, in.dA, rc, in.D, in.Qp, rd1, rd2, lg1, lg2);
    }
};
// psi2 (M x M, ld M) of all rows into out (device), chunk by chunk in row order
int psi2_all(hipStream_t st, const PsiInputs& in, PsiRows& rw, double* part, long ld, double* out) {
    int nch = 0;
    for (long r0 = 0; r0 < in.N; r0 += PSI_CHUNK, ++nch) {
        const long rc = (in.N - r0 < PSI_CHUNK) ? (in.N - r0) : PSI_CHUNK;
        rw.fill(st, in, r0, rc);
        const int ns = launch_psi2(st, rw.rd2, rw.lg2, in.dW ? in.dW + r0 : nullptr, in.dZp, in.dA, rc, in.M, in.Qp,
                                   in.var * in.var, ld, part);
        launch_psi2_combine(st, part, ld, in.M, ns, nch > 0, out, in.M);
    }
    return 0;
}
}  // namespace

extern "C" {

// psi1 (N x M) and / or psi2 = sum_n w_n psi2n (M x M) of an RBF kernel (lengthscale: D entries if ard, else one)
int mi355gp_rbf_psi(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                    const double* mu, const double* S, int64_t N, int D, const double* weights, double* psi1_out,
                    double* psi2_out) {
    HIP_CHECK(hipSetDevice(device));
    PsiInputs in;
    if (int rc = in.load("mi355gp_rbf_psi", variance, lengthscale, ard, Z, M, mu, S, N, D, weights)) return rc;
    hipStream_t st = 0;
    const long chunk = N < PSI_CHUNK ? N : PSI_CHUNK, ld = round_up(M, PSI_T2);
    PsiRows rw;
    if (int rc = rw.alloc(chunk, in.Qp)) return rc;
    if (psi1_out) {
        DevBuf d1;
        HIP_CHECK(d1.alloc(chunk * M));
        for (long r0 = 0; r0 < N; r0 += PSI_CHUNK) {
            const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
            rw.fill(st, in, r0, rc);
            launch_psi1(st, rw.rd1, rw.lg1, in.dZp, rc, (long)M, in.mpad, in.Qp, variance, d1, (long)M);
            HIP_CHECK(hipMemcpy(psi1_out + r0 * M, d1, sizeof(double) * rc * M, hipMemcpyDeviceToHost));
        }
    }
    if (psi2_out) {
        DevBuf part, d2;
        HIP_CHECK(part.alloc((size_t)psi2_nsplit(chunk, M) * ld * ld));
        HIP_CHECK(d2.alloc(M * M));
        if (int rc = psi2_all(st, in, rw, part, ld, d2)) return rc;
        HIP_CHECK(hipMemcpy(psi2_out, d2, sizeof(double) * M * M, hipMemcpyDeviceToHost));
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    return 0;
}

// The five outputs of psiDerivativecomputations (rbf_psi_comp.py:70-133) from dL_dpsi0 (N), dL_dpsi1 (N x M), dL_dpsi2
// (M x M, symmetrised here); each may be NULL.  weights (N, optional): psi2 = sum_n w_n psi2n.
// dl_out: D entries if ard, else one; dZ_out M x D; dmu_out, dS_out N x D.
int mi355gp_rbf_psi_grad(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                         const double* mu, const double* S, int64_t N, int D, const double* weights, const double* dL_dpsi0,
                         const double* dL_dpsi1, const double* dL_dpsi2, double* dvar_out, double* dl_out, double* dZ_out,
                         double* dmu_out, double* dS_out) {
    ARG_CHECK(dvar_out && dl_out && dZ_out && dmu_out && dS_out, "mi355gp_rbf_psi_grad: NULL output");
    HIP_CHECK(hipSetDevice(device));
    PsiInputs in;
    if (int rc = in.load("mi355gp_rbf_psi_grad", variance, lengthscale, ard, Z, M, mu, S, N, D, weights)) return rc;
    hipStream_t st = 0;
    const int Qp = in.Qp, RL = 1 + 2 * Qp;
    const long chunk = N < PSI_CHUNK ? N : PSI_CHUNK, ld = round_up(M, PSI_T2), mpad = in.mpad, mt = (M + 15) / 16;
    const long nzb = (chunk + PSI_GROWS - 1) / PSI_GROWS;
    PsiRows rw;
    if (int rc = rw.alloc(chunk, Qp)) return rc;
    DevBuf dG, dL2, dPsi2, part, Ppart, P1s, P2s, Zpart, Zs1, Zs2, dMuO, dSO, rowrec, rec, zz;
    std::vector<double> zs1((size_t)mpad * Qp, 0.0), zs2((size_t)mpad * Qp, 0.0), zzh((size_t)M * 2 * Qp, 0.0);
    std::vector<double> sums((size_t)(1 + Qp), 0.0), csum((size_t)(1 + Qp));
    HIP_CHECK(Ppart.alloc((size_t)mt * chunk * RL));
    HIP_CHECK(P1s.alloc((size_t)chunk * RL));
    HIP_CHECK(P2s.alloc((size_t)chunk * RL));
    HIP_CHECK(Zpart.alloc((size_t)nzb * mpad * Qp));
    HIP_CHECK(hipMemset(Zpart, 0, sizeof(double) * nzb * mpad * Qp));       // the kernels write rows < round_up(M, 16) only
    HIP_CHECK(Zs1.alloc((size_t)mpad * Qp));
    HIP_CHECK(Zs2.alloc((size_t)mpad * Qp));
    HIP_CHECK(dMuO.alloc(chunk * D));
    HIP_CHECK(dSO.alloc(chunk * D));
    HIP_CHECK(rowrec.alloc((size_t)chunk * (1 + Qp)));
    HIP_CHECK(rec.alloc(1 + Qp));
    if (dL_dpsi1) HIP_CHECK(dG.alloc(chunk * M));
    if (dL_dpsi2) {
        // psi2 first (LS = dL_dpsi2 * psi2 carries the z_m - z_o terms), then the symmetrised dL_dpsi2 for the row passes
        HIP_CHECK(part.alloc((size_t)psi2_nsplit(chunk, M) * ld * ld));     // (>= 1: also holds dL_dpsi2, M x M)
        HIP_CHECK(dPsi2.alloc(M * M));
        HIP_CHECK(dL2.alloc(M * M));
        HIP_CHECK(zz.alloc((size_t)M * 2 * Qp));
        if (int rc = psi2_all(st, in, rw, part, ld, dPsi2)) return rc;
        HIP_CHECK(hipMemcpy(part, dL_dpsi2, sizeof(double) * M * M, hipMemcpyHostToDevice));      // (part: free again)
        hipLaunchKernelGGL(k_psi_symmetrise, dim3((unsigned)((M + 255) / 256), (unsigned)M), dim3(256), 0, st, part.p, (long)M, dL2.p);
        launch_psi2_zz(st, dL2, dPsi2, (long)M, in.dZp, (long)M, Qp, zz);
        HIP_CHECK(hipMemcpy(zzh.data(), zz, sizeof(double) * zzh.size(), hipMemcpyDeviceToHost));
    }
    int nch = 0;
    for (long r0 = 0; r0 < N; r0 += PSI_CHUNK, ++nch) {
        const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
        const int nb = (int)((rc + PSI_GROWS - 1) / PSI_GROWS);
        rw.fill(st, in, r0, rc);
        if (dL_dpsi1) {
            HIP_CHECK(hipMemcpy(dG, dL_dpsi1 + r0 * M, sizeof(double) * rc * M, hipMemcpyHostToDevice));
            launch_psi1_grad(st, rw.rd1, rw.lg1, in.dZp, dG, M, PsiRank{nullptr, nullptr, 0, 0.0}, rc, M, mpad, Qp, variance, Ppart,
                             Zpart);
            launch_sum_splits(st, Ppart, rc * RL, (int)mt, 0, P1s);
            launch_sum_splits(st, Zpart, mpad * Qp, nb, nch > 0, Zs1);
        }
        if (dL_dpsi2) {
            launch_psi2_grad(st, rw.rd2, rw.lg2, in.dW ? in.dW + r0 : nullptr, in.dZp, in.dA, dL2, M, rc, M, mpad,
                             Qp, variance * variance, Ppart, Zpart);
            launch_sum_splits(st, Ppart, rc * RL, (int)mt, 0, P2s);
            launch_sum_splits(st, Zpart, mpad * Qp, nb, nch > 0, Zs2);
        }
        launch_psi_rowfinish(st, dL_dpsi1 ? (const double*)P1s.p : nullptr, dL_dpsi2 ? (const double*)P2s.p : nullptr,
                             in.dS + r0 * D, in.dA, rc, D, Qp, dMuO, dSO, rowrec);
        launch_reduce_partials(st, rowrec, (int)rc, 1 + Qp, rec);
        HIP_CHECK(hipMemcpy(dmu_out + r0 * D, dMuO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(dS_out + r0 * D, dSO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(csum.data(), rec, sizeof(double) * (1 + Qp), hipMemcpyDeviceToHost));
        for (int k = 0; k <= Qp; ++k) sums[(size_t)k] += csum[(size_t)k];                          // chunks in row order
    }
    if (dL_dpsi1) HIP_CHECK(hipMemcpy(zs1.data(), Zs1, sizeof(double) * zs1.size(), hipMemcpyDeviceToHost));
    if (dL_dpsi2) HIP_CHECK(hipMemcpy(zs2.data(), Zs2, sizeof(double) * zs2.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    // dZ = sum_n c1 L1 d  +  2 sum_{n,o} c2 L2 d  -  a_q sum_o LS (z_m - z_o)      (dL_dpsi2 symmetric: both positions of z_m)
    for (long i = 0; i < M; ++i)
        for (int q = 0; q < D; ++q)
            dZ_out[i * D + q] = zs1[(size_t)i * Qp + q] + 2.0 * zs2[(size_t)i * Qp + q] - in.a[(size_t)q] * zzh[(size_t)i * 2 * Qp + q];
    // variance and lengthscales through the reduction records of the kernel gradients (part_dtheta: dl = -rec / l)
    const int groups = (D + 31) / 32;
    std::vector<double> recs((size_t)groups * GP_STRIDE, 0.0), th(in.spec.theta.size());
    double v0 = sums[0];
    if (dL_dpsi0)
        for (int64_t i = 0; i < N; ++i) v0 += dL_dpsi0[i] * variance;                              // psi0 = variance
    recs[0] = v0;
    for (int q = 0; q < D; ++q) {
        double zq = 0.0;
        for (long i = 0; i < M; ++i) zq += zzh[(size_t)i * 2 * Qp + Qp + q];
        const double lq = sums[(size_t)(1 + q)] + 0.5 * in.a[(size_t)q] * zq;                      // 2 * a dz^2 / 4 summed over (m, o)
        recs[(size_t)(q / 32) * GP_STRIDE + 2 + (q % 32)] = -lq;
        recs[1] -= lq;
    }
    part_dtheta(in.spec, recs.data(), nullptr, th.data());
    *dvar_out = th[0];
    for (size_t k = 1; k < th.size(); ++k) dl_out[k - 1] = th[k];
    return 0;
}

}  // extern "C"
