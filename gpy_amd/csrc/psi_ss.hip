// psi_ss.hip -- psi-statistics of the RBF kernel for spike-and-slab inputs q(x_nq) = g_nq N(mu_nq, S_nq) + (1 - g_nq) delta_0,
// and their gradients.  Restates (does not port) GPy/kern/src/psi_comp/ssrbf_psi_comp.py, the computation the reference also
// wrote device code for (ssrbf_psi_gpucomp.py).  With a_q = 1 / l_q^2, c1 = a / (S a + 1), c2 = a / (2 S a + 1),
// E[m,q] = exp(-a_q z_mq^2 / 2):
//   psi1[n,m]  = var   prod_q f1,  f1 = g (S a + 1)^-1/2  exp(-c1 (mu - z_m)^2 / 2)                        + (1 - g) E[m,q]
//   psi2n[m,o] = var^2 prod_q f2,  f2 = g (2 S a + 1)^-1/2 exp(-a (z_m - z_o)^2/4 - c2 (mu - (z_m+z_o)/2)^2) + (1 - g) E[m,q] E[o,q]
// The product of two-term factors does not collapse into one exponent: one fp64 exp per (element, q), where the Gaussian
// kernels of psi.hip have one per element.  The padding and a dimension with a = 0 have f = 1 exactly (record (0, 0, 1, 0)).
// Squared differences are evaluated directly, every sum over n, m or o is combined in a fixed order (psi.hip), psi2 is built
// on lower 16-tiles and mirrored.
//
// Gradients.  With L = dL * psi per element, s the slab term of f, rho = s / f and sig = 1 - rho = (spike term) / f, both 0
// where f underflowed to 0 (then L is 0 too: the element contributes exactly 0), the gradient kernels produce
//   per row n and dimension q     R0 = sum L rho, R1 = sum L rho d, R2 = sum L rho d^2, K0 = sum L sig   (and P0 = sum L)
//   per inducing point m and q    Zs = sum L rho (d/dz_m of the slab exponent), Zk = sum L sig, Zq = sum L rho (z_m - z_o)^2
// psi2n is recomputed tile by tile.  k_pss_rowfinish turns the row sums into dmu, dS, dgamma and the per-row variance /
// lengthscale sums:  dgamma = R0 / g - K0 / (1 - g)  (K0 is summed on its own: P0 - R0 cancels for g near 1).  The spike
// share reaches Z as -a z_m Zk and the lengthscale as a z_m^2 Zk.
#include <cmath>
#include <vector>

#include "../../include/mi355gp_psi_ss.h"
#include "internal.h"
#include "parts.h"
#include "psi_ss.h"

#define PSS_DC 16              // dimensions psi1 stages at a time; width of one accumulator group of the psi1 gradient kernel
#define PSS_DC2 8              // ... of the psi2 gradient kernel (seven sums per dimension: 16 dimensions spill)

// per row: r1[n][q] = (mu, c1, g (S a + 1)^-1/2, 1 - g), r2[n][q] = (mu, c2, g (2 S a + 1)^-1/2, 1 - g); (0, 0, 1, 0) where a = 0
__global__ void k_pss_rows(const double* __restrict__ mu, const double* __restrict__ S, const double* __restrict__ gam,
                           const double* __restrict__ a, long rows, int D, int Qp, double4* __restrict__ r1,
                           double4* __restrict__ r2) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    for (int q = 0; q < Qp; ++q) {
        double4 v1 = make_double4(0.0, 0.0, 1.0, 0.0), v2 = v1;
        if (q < D && a[q] > 0.0) {
            const double aq = a[q], m = mu[n * D + q], s = S[n * D + q], g = gam[n * D + q];
            const double d1 = fma(s, aq, 1.0), d2 = fma(2.0 * s, aq, 1.0);
            v1 = make_double4(m, aq / d1, g / sqrt(d1), 1.0 - g);
            v2 = make_double4(m, aq / d2, g / sqrt(d2), 1.0 - g);
        }
        r1[n * Qp + q] = v1;
        r2[n * Qp + q] = v2;
    }
}

// Ep[m][q] = exp(-a_q z_mq^2 / 2) over the padded Z (1 in the padding)
__global__ void k_pss_e(const double* __restrict__ Zp, const double* __restrict__ a, long cnt, int Qp, double* __restrict__ Ep) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const double z = Zp[i];
    Ep[i] = exp(-0.5 * (a[i % Qp] * z) * z);
}

// psi1 tile: 64 rows x 64 inducing points, thread = one column and 16 rows, dimensions in groups of PSS_DC (48 KB of LDS)
__global__ __launch_bounds__(256) void k_pss_psi1(const double4* __restrict__ rd, const double* __restrict__ Zp,
                                                  const double* __restrict__ Ep, long rows, long m, int Qp, double var,
                                                  double* __restrict__ out, long ldo) {
    __shared__ double4 rs[PSI_KT * PSS_DC];
    __shared__ double zs[PSI_KT * (PSS_DC + 1)], es[PSI_KT * (PSS_DC + 1)];
    const int t = threadIdx.x, mc = t & 63, g = t >> 6;
    const long n0 = (long)blockIdx.x * PSI_KT, m0 = (long)blockIdx.y * PSI_KT;
    double pr[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) pr[k] = 1.0;
    for (int qg = 0; qg < Qp; qg += PSS_DC) {
        const int qn = (Qp - qg < PSS_DC) ? (Qp - qg) : PSS_DC;
        for (int idx = t; idx < PSI_KT * qn; idx += 256) {
            const int r = idx / qn, q = idx - r * qn;
            zs[r * (PSS_DC + 1) + q] = Zp[(m0 + r) * Qp + qg + q];
            es[r * (PSS_DC + 1) + q] = Ep[(m0 + r) * Qp + qg + q];
            rs[r * PSS_DC + q] = (n0 + r < rows) ? rd[(n0 + r) * Qp + qg + q] : make_double4(0.0, 0.0, 1.0, 0.0);
        }
        __syncthreads();
        for (int q = 0; q < qn; ++q) {
            const double z = zs[mc * (PSS_DC + 1) + q], e = es[mc * (PSS_DC + 1) + q];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const double4 v = rs[(g * 16 + k) * PSS_DC + q];
                const double d = v.x - z;
                pr[k] *= fma(v.z, exp(-0.5 * (v.y * d) * d), v.w * e);
            }
        }
        __syncthreads();
    }
    if (m0 + mc >= m) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const long n = n0 + g * 16 + k;
        if (n < rows) out[n * ldo + m0 + mc] = var * pr[k];
    }
}

// psi2 partial sums, the layout of k_psi2: part[split][mi][oj] (ld x ld, lower 16-tiles).  Thread = one (m, o); its
// row-independent operands -- the midpoint, a dz^2 / 4 (it joins the slab exponent: one exp per factor) and E[m] E[o] -- are
// computed once, before the rows.  At QP = 64 the three vectors do not fit in registers: the dimensions are walked in two
// groups of PSI_KDC, the first group's product of every staged row waits in LDS (pr, read back by the thread that wrote it),
// and the three vectors of a group are formed again per row block of 16 (no exponentials in them).
template <int QP>
__global__ __launch_bounds__(256) void k_pss_psi2(const double4* __restrict__ rd2, const double* __restrict__ w,
                                                  const double* __restrict__ Zp, const double* __restrict__ Ep,
                                                  const double* __restrict__ ap, long rows, long rps, long m, double var2,
                                                  long ld, double* __restrict__ part) {
    constexpr int QG = QP > PSI_KDC ? PSI_KDC : QP, NG = QP / QG, RB = QP >= 32 ? 16 : 64;
    __shared__ double4 rs[RB * QG];
    __shared__ double ws[RB];
    __shared__ double pr[NG > 1 ? RB * 256 : 1];
    int ti, tj;
    psi_tile(blockIdx.x, &ti, &tj);
    const int t = threadIdx.x;
    const long mi = (long)ti * PSI_T2 + (t >> 4), oj = (long)tj * PSI_T2 + (t & 15);
    double zq[QG], zb[QG], ee[QG];
    if (NG == 1) {
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const double zm = Zp[mi * QP + q], zo = Zp[oj * QP + q], dz = zm - zo;
            zq[q] = 0.25 * (ap[q] * dz) * dz;
            zb[q] = 0.5 * (zm + zo);
            ee[q] = Ep[mi * QP + q] * Ep[oj * QP + q];
        }
    }
    const long r0 = (long)blockIdx.y * rps, r1 = (r0 + rps < rows) ? (r0 + rps) : rows;
    double acc = 0.0;
    for (long rb = r0; rb < r1; rb += RB) {
#pragma unroll 1                                               // (unrolled, both groups' vectors are hoisted out of the row loop and spill)
        for (int g = 0; g < NG; ++g) {
            if (NG > 1) {
#pragma unroll
                for (int q = 0; q < QG; ++q) {
                    const double zm = Zp[mi * QP + g * QG + q], zo = Zp[oj * QP + g * QG + q], dz = zm - zo;
                    zq[q] = 0.25 * (ap[g * QG + q] * dz) * dz;
                    zb[q] = 0.5 * (zm + zo);
                    ee[q] = Ep[mi * QP + g * QG + q] * Ep[oj * QP + g * QG + q];
                }
            }
            __syncthreads();                                   // the last group's reads of rs / ws are done
            for (int idx = t; idx < RB * QG; idx += 256) {
                const long n = rb + idx / QG;
                rs[idx] = (n < r1) ? rd2[n * QP + g * QG + (idx % QG)] : make_double4(0.0, 0.0, 1.0, 0.0);
            }
            if (g == 0 && t < RB) {
                const long n = rb + t;
                ws[t] = (n < r1) ? (w ? w[n] : 1.0) : 0.0;
            }
            __syncthreads();
            for (int r = 0; r < RB; ++r) {
                double p = 1.0;
#pragma unroll
                for (int q = 0; q < QG; ++q) {
                    const double4 v = rs[r * QG + q];
                    const double d = v.x - zb[q];
                    p *= fma(v.z, exp(-fma(v.y * d, d, zq[q])), v.w * ee[q]);
                    __builtin_amdgcn_sched_barrier(0);         // one factor at a time: interleaved exponentials spill
                }
                if (NG == 1) acc = fma(ws[r], p, acc);
                else if (g == 0) pr[r * 256 + t] = p;
                else acc = fma(ws[r], pr[r * 256 + t] * p, acc);
            }
        }
    }
    if (mi < m && oj < m) part[(long)blockIdx.y * ld * ld + mi * ld + oj] = var2 * acc;
}

// ---- gradient kernels ------------------------------------------------------------------------------------------------
// Both: workgroup = 16 inducing points (ml = lane & 15) x 16 rows at a time (nl = thread >> 4), PSI_GROWS rows in all;
// blockIdx.z = accumulator group of PSS_DC (psi1) or PSS_DC2 (psi2) dimensions.  The product always runs over all Qp dimensions; the group's factors
// are then evaluated again for their shares (Qp + QG exponentials per element and group).
//   Ppart[mtile][row][1 + 4 Qp]: P0, R0[q], R1[q], R2[q], K0[q] summed over the tile's 16 inducing points (lane shuffles)
//   Zpart[rowblock][m][3 Qp]:    Zs[q], Zk[q], Zq[q] summed over the block's rows (and all o)
// LDS (dynamic): rows 16 x Qp double4 | zm, em 16 x (Qp + 1) | (psi2 only) aq Qp, zo, eo OC x Qp, dLs OC x 16; the reduction
// of the Z sums (4 x 16 x 3 QG) reuses the front of it.
__device__ __forceinline__ double pss_sum16(double v) {        // over the 16 lanes that share a row (fixed tree)
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

// sum zacc over the 16 rows of the workgroup (4 per wave by shuffles, 4 waves through LDS in wave order) and store
template <int QG>
__device__ __forceinline__ void pss_emit_z(int t, int qoff, int Qp, long mcol, long mpad, double* zacc, double* zred,
                                           double* __restrict__ zblock) {
#pragma unroll
    for (int q = 0; q < PSS_NZ * QG; ++q) {
        zacc[q] += __shfl_xor(zacc[q], 16);
        zacc[q] += __shfl_xor(zacc[q], 32);
    }
    const int lane = t & 63, wv = t >> 6;
    if (lane < 16)
#pragma unroll
        for (int q = 0; q < PSS_NZ * QG; ++q) zred[(wv * 16 + lane) * PSS_NZ * QG + q] = zacc[q];
    __syncthreads();
    if (t < 16 && mcol < mpad)
#pragma unroll
        for (int k = 0; k < PSS_NZ; ++k)
#pragma unroll
            for (int q = 0; q < QG; ++q) {
                const int j = k * QG + q;
                const double s = (zred[(0 * 16 + t) * PSS_NZ * QG + j] + zred[(1 * 16 + t) * PSS_NZ * QG + j]) +
                                 (zred[(2 * 16 + t) * PSS_NZ * QG + j] + zred[(3 * 16 + t) * PSS_NZ * QG + j]);
                zblock[mcol * PSS_NZ * Qp + k * Qp + qoff + q] = s;
            }
}

// psi1: L = G[n][m] var prod_q f1, d = mu - z_m; Zs = sum c1 L rho d.  G == NULL: the weights are rk's product beta R_n . v_m
template <int QG>
__global__ __launch_bounds__(256) void k_pss_psi1_grad(const double4* __restrict__ rd, const double* __restrict__ Zp,
                                                       const double* __restrict__ Ep, const double* __restrict__ G, long ldg,
                                                       PsiRank rk, long rows, long m, long mpad, int Qp, double var,
                                                       double* __restrict__ Ppart, double* __restrict__ Zpart) {
    extern __shared__ __align__(32) double sm[];
    double4* rs = (double4*)sm;                                // 16 x Qp
    double* zm = sm + 64 * Qp;                                 // 16 x (Qp + 1)
    double* em = zm + 16 * (Qp + 1);                           // 16 x (Qp + 1)
    const int t = threadIdx.x, ml = t & 15, nl = t >> 4, gz = blockIdx.z, qoff = gz * PSS_DC;
    const long mcol = (long)blockIdx.x * 16 + ml, nb0 = (long)blockIdx.y * PSI_GROWS;
    const int RL = 1 + 4 * Qp;
    for (int idx = t; idx < 16 * Qp; idx += 256) {
        const int r = idx / Qp, q = idx - r * Qp;
        zm[r * (Qp + 1) + q] = Zp[((long)blockIdx.x * 16 + r) * Qp + q];
        em[r * (Qp + 1) + q] = Ep[((long)blockIdx.x * 16 + r) * Qp + q];
    }
    double zacc[PSS_NZ * QG];
#pragma unroll
    for (int q = 0; q < PSS_NZ * QG; ++q) zacc[q] = 0.0;
    for (int it = 0; it < PSI_GROWS / 16; ++it) {
        const long nbase = nb0 + it * 16;
        if (nbase >= rows) break;                              // (uniform over the workgroup)
        __syncthreads();
        for (int idx = t; idx < 16 * Qp; idx += 256) {
            const long n = nbase + idx / Qp;
            rs[idx] = (n < rows) ? rd[n * Qp + (idx % Qp)] : make_double4(0.0, 0.0, 1.0, 0.0);
        }
        __syncthreads();
        const long n = nbase + nl;
        const bool ok = n < rows && mcol < m;
        double p = 1.0;
        for (int q = 0; q < Qp; ++q) {
            const double4 v = rs[nl * Qp + q];
            const double d = v.x - zm[ml * (Qp + 1) + q];
            p *= fma(v.z, exp(-0.5 * (v.y * d) * d), v.w * em[ml * (Qp + 1) + q]);
        }
        double gw = 0.0;                                       // dL_dpsi1[n][m]: given, or beta R_n . v_m formed here
        if (ok) {
            if (G) gw = G[n * ldg + mcol];
            else {
                for (int d = 0; d < rk.Dy; ++d) gw = fma(rk.R[n * rk.Dy + d], rk.v[mcol * rk.Dy + d], gw);
                gw *= rk.beta;
            }
        }
        const double L = gw * var * p;
        double* prow = Ppart + ((long)blockIdx.x * rows + (n < rows ? n : 0)) * RL;
        const bool st = ml == 0 && n < rows;
        const double a0 = pss_sum16(L);
        if (st && gz == 0) prow[0] = a0;
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const double4 v = rs[nl * Qp + qoff + q];
            const double d = v.x - zm[ml * (Qp + 1) + qoff + q];
            const double s = v.z * exp(-0.5 * (v.y * d) * d), k = v.w * em[ml * (Qp + 1) + qoff + q], f = s + k;
            const double Lr = f > 0.0 ? L * (s / f) : 0.0, Lk = f > 0.0 ? L * (k / f) : 0.0;
            const double g1 = Lr * d, g2 = g1 * d;
            zacc[q] = fma(v.y, g1, zacc[q]);
            zacc[QG + q] += Lk;
            const double s0 = pss_sum16(Lr), s1 = pss_sum16(g1), s2 = pss_sum16(g2), s3 = pss_sum16(Lk);
            if (st) {
                prow[1 + qoff + q] = s0;
                prow[1 + Qp + qoff + q] = s1;
                prow[1 + 2 * Qp + qoff + q] = s2;
                prow[1 + 3 * Qp + qoff + q] = s3;
            }
        }
    }
    __syncthreads();                                           // rs is free: the Z reduction reuses it
    pss_emit_z<QG>(t, qoff, Qp, mcol, mpad, zacc, sm, Zpart + (long)blockIdx.y * mpad * PSS_NZ * Qp);
}

// psi2: L = w_n dL[m][o] var^2 prod_q f2, d = mu - (z_m + z_o)/2, dz = z_m - z_o; dL symmetric, read as dL[o][m];
// Zs = sum L rho (c2 d - a dz / 2), Zq = sum L rho dz^2
template <int QG>
__global__ __launch_bounds__(256) void k_pss_psi2_grad(const double4* __restrict__ rd, const double* __restrict__ w,
                                                       const double* __restrict__ Zp, const double* __restrict__ Ep,
                                                       const double* __restrict__ ap, const double* __restrict__ dL, long ldd,
                                                       long rows, long m, long mpad, int Qp, int OC, double var2,
                                                       double* __restrict__ Ppart, double* __restrict__ Zpart) {
    extern __shared__ __align__(32) double sm[];
    double4* rs = (double4*)sm;                                // 16 x Qp
    double* zm = sm + 64 * Qp;                                 // 16 x (Qp + 1)
    double* em = zm + 16 * (Qp + 1);                           // 16 x (Qp + 1)
    double* aq = em + 16 * (Qp + 1);                           // Qp
    double* zo = aq + Qp;                                      // OC x Qp
    double* eo = zo + OC * Qp;                                 // OC x Qp
    double* dLs = eo + OC * Qp;                                // OC x 16: dL[o][m] var^2
    const int t = threadIdx.x, ml = t & 15, nl = t >> 4, gz = blockIdx.z, qoff = gz * PSS_DC2;
    const long mcol = (long)blockIdx.x * 16 + ml, nb0 = (long)blockIdx.y * PSI_GROWS;
    const int RL = 1 + 4 * Qp;
    for (int idx = t; idx < 16 * Qp; idx += 256) {
        const int r = idx / Qp, q = idx - r * Qp;
        zm[r * (Qp + 1) + q] = Zp[((long)blockIdx.x * 16 + r) * Qp + q];
        em[r * (Qp + 1) + q] = Ep[((long)blockIdx.x * 16 + r) * Qp + q];
    }
    for (int q = t; q < Qp; q += 256) aq[q] = ap[q];
    double zacc[PSS_NZ * QG];
#pragma unroll
    for (int q = 0; q < PSS_NZ * QG; ++q) zacc[q] = 0.0;
    for (int it = 0; it < PSI_GROWS / 16; ++it) {
        const long nbase = nb0 + it * 16;
        if (nbase >= rows) break;
        __syncthreads();
        for (int idx = t; idx < 16 * Qp; idx += 256) {
            const long n = nbase + idx / Qp;
            rs[idx] = (n < rows) ? rd[n * Qp + (idx % Qp)] : make_double4(0.0, 0.0, 1.0, 0.0);
        }
        const long n = nbase + nl;
        const bool nok = n < rows;
        const double wn = nok ? (w ? w[n] : 1.0) : 0.0;
        double a0 = 0.0, r0[QG], r1[QG], r2[QG], k0[QG];
#pragma unroll
        for (int q = 0; q < QG; ++q) r0[q] = r1[q] = r2[q] = k0[q] = 0.0;
        for (long oc = 0; oc < m; oc += OC) {
            const int on = (m - oc < OC) ? (int)(m - oc) : OC;
            __syncthreads();                                   // (also orders the stores of zm / em / aq / rs before their first use)
            for (int idx = t; idx < on * Qp; idx += 256) {
                zo[idx] = Zp[oc * Qp + idx];
                eo[idx] = Ep[oc * Qp + idx];
            }
            for (int idx = t; idx < on * 16; idx += 256) {
                const long mc = (long)blockIdx.x * 16 + (idx & 15);
                dLs[idx] = (mc < m) ? dL[(oc + (idx >> 4)) * ldd + mc] * var2 : 0.0;
            }
            __syncthreads();
            for (int o = 0; o < on; ++o) {
                double p = 1.0;
                for (int q = 0; q < Qp; ++q) {
                    const double4 v = rs[nl * Qp + q];
                    const double z1 = zm[ml * (Qp + 1) + q], z2 = zo[o * Qp + q], dz = z1 - z2, d = v.x - 0.5 * (z1 + z2);
                    p *= fma(v.z, exp(-fma(v.y * d, d, 0.25 * (aq[q] * dz) * dz)), v.w * (em[ml * (Qp + 1) + q] * eo[o * Qp + q]));
                }
                const double L = dLs[o * 16 + ml] * wn * p;
                a0 += L;
#pragma unroll
                for (int q = 0; q < QG; ++q) {
                    const int qq = qoff + q;
                    const double4 v = rs[nl * Qp + qq];
                    const double z1 = zm[ml * (Qp + 1) + qq], z2 = zo[o * Qp + qq], dz = z1 - z2, d = v.x - 0.5 * (z1 + z2);
                    const double s = v.z * exp(-fma(v.y * d, d, 0.25 * (aq[qq] * dz) * dz));
                    const double k = v.w * (em[ml * (Qp + 1) + qq] * eo[o * Qp + qq]), f = s + k;
                    const double Lr = f > 0.0 ? L * (s / f) : 0.0, Lk = f > 0.0 ? L * (k / f) : 0.0;
                    const double Ld = Lr * d;
                    r0[q] += Lr;
                    r1[q] += Ld;
                    r2[q] = fma(Ld, d, r2[q]);
                    k0[q] += Lk;
                    zacc[q] = fma(Lr, fma(v.y, d, -0.5 * aq[qq] * dz), zacc[q]);
                    zacc[QG + q] += Lk;
                    zacc[2 * QG + q] = fma(Lr * dz, dz, zacc[2 * QG + q]);
                    __builtin_amdgcn_sched_barrier(0);         // one dimension at a time: interleaved exponentials spill
                }
            }
        }
        double* prow = Ppart + ((long)blockIdx.x * rows + (nok ? n : 0)) * RL;
        const bool st = ml == 0 && nok;
        a0 = pss_sum16(a0);
        if (st && gz == 0) prow[0] = a0;
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const double s0 = pss_sum16(r0[q]), s1 = pss_sum16(r1[q]), s2 = pss_sum16(r2[q]), s3 = pss_sum16(k0[q]);
            if (st) {
                prow[1 + qoff + q] = s0;
                prow[1 + Qp + qoff + q] = s1;
                prow[1 + 2 * Qp + qoff + q] = s2;
                prow[1 + 3 * Qp + qoff + q] = s3;
            }
        }
    }
    __syncthreads();                                           // the staged operands are free: the Z reduction reuses them
    pss_emit_z<QG>(t, qoff, Qp, mcol, mpad, zacc, sm, Zpart + (long)blockIdx.y * mpad * PSS_NZ * Qp);
}

// rows of the chunk: dmu, dS, dgamma (n x D, stored) and rowrec[n][1 + Qp] = {variance sum, lengthscale sums} from the summed
// row records of psi1 (P1s) and psi2 (P2s), either may be NULL.  With d1 = S a + 1, d2 = 2 S a + 1:
//   psi1: dmu = -c1 R1, dS = (c1^2 R2 - c1 R0)/2,  l_q dE/dl_q = c1 S R0 + (c1/d1) R2,       variance sum P0
//   psi2: dmu = -2 c2 R1, dS = 2 c2^2 R2 - c2 R0,  l_q dE/dl_q = 2 (c2 S R0 + (c2/d2) R2),   variance sum 2 P0
//   both: dgamma = R0 / g - K0 / (1 - g).  A dimension with a = 0 gets exactly 0.0 in all three.
__global__ void k_pss_rowfinish(const double* __restrict__ P1s, const double* __restrict__ P2s, const double* __restrict__ S,
                                const double* __restrict__ gam, const double* __restrict__ a, long rows, int D, int Qp,
                                double* __restrict__ dmu, double* __restrict__ dS, double* __restrict__ dgam,
                                double* __restrict__ rowrec) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    const int RL = 1 + 4 * Qp;
    const double p01 = P1s ? P1s[n * RL] : 0.0, p02 = P2s ? P2s[n * RL] : 0.0;
    rowrec[n * (1 + Qp)] = p01 + 2.0 * p02;
    for (int q = 0; q < Qp; ++q) {
        double gm = 0.0, gs = 0.0, gg = 0.0, gl = 0.0;
        if (q < D) {
            const double aq = a[q], s = S[n * D + q], g = gam[n * D + q];
            if (aq > 0.0) {
                if (P1s) {
                    const double* P = P1s + n * RL + 1 + q;
                    const double d1 = fma(s, aq, 1.0), c1 = aq / d1, R0 = P[0], R1 = P[Qp], R2 = P[2 * Qp], K0 = P[3 * Qp];
                    gm -= c1 * R1;
                    gs += 0.5 * (c1 * c1 * R2 - c1 * R0);
                    gg += R0 / g - K0 / (1.0 - g);
                    gl += c1 * s * R0 + (c1 / d1) * R2;
                }
                if (P2s) {
                    const double* P = P2s + n * RL + 1 + q;
                    const double d2 = fma(2.0 * s, aq, 1.0), c2 = aq / d2, R0 = P[0], R1 = P[Qp], R2 = P[2 * Qp], K0 = P[3 * Qp];
                    gm -= 2.0 * c2 * R1;
                    gs += 2.0 * c2 * c2 * R2 - c2 * R0;
                    gg += R0 / g - K0 / (1.0 - g);
                    gl += 2.0 * (c2 * s * R0 + (c2 / d2) * R2);
                }
            }
            dmu[n * D + q] = gm;
            dS[n * D + q] = gs;
            dgam[n * D + q] = gg;
        }
        rowrec[n * (1 + Qp) + 1 + q] = gl;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
template <int QP>
static void launch_pss_psi2_t(hipStream_t st, const double4* rd2, const double* w, const double* Zp, const double* Ep,
                              const double* ap, long rows, long m, double var2, long ld, int nsplit, double* part) {
    const long nt = (m + PSI_T2 - 1) / PSI_T2, ntl = nt * (nt + 1) / 2;
    const long rps = round_up((rows + nsplit - 1) / nsplit, 64);
    hipLaunchKernelGGL((k_pss_psi2<QP>), dim3((unsigned)ntl, (unsigned)nsplit), dim3(256), 0, st, rd2, w, Zp, Ep, ap, rows, rps,
                       m, var2, ld, part);
}
int launch_pss_psi2(hipStream_t st, const double* rd2_, const double* w, const double* Zp, const double* Ep, const double* ap,
                    long rows, long m, int Qp, double var2, long ld, double* part) {
    const double4* rd2 = (const double4*)rd2_;
    const int ns = psi2_nsplit(rows, m);
    switch (Qp) {
        case 1: launch_pss_psi2_t<1>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
        case 2: launch_pss_psi2_t<2>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
        case 4: launch_pss_psi2_t<4>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
        case 8: launch_pss_psi2_t<8>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
        case 16: launch_pss_psi2_t<16>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
        case 32: launch_pss_psi2_t<32>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
        default: launch_pss_psi2_t<64>(st, rd2, w, Zp, Ep, ap, rows, m, var2, ld, ns, part); break;
    }
    return ns;
}

static int pss_oc(int Qp) { return Qp > 32 ? 8 : 32; }       // inducing points o the psi2 gradient kernel stages at a time
static size_t pss_grad_lds(int Qp, int QG, bool second) {
    size_t d = 64 * (size_t)Qp + 2 * 16 * ((size_t)Qp + 1);
    if (second) d += (size_t)Qp + 2 * (size_t)pss_oc(Qp) * Qp + (size_t)pss_oc(Qp) * 16;
    const size_t zred = 4 * 16 * PSS_NZ * (size_t)QG;
    return (d > zred ? d : zred) * sizeof(double);             // at most 58 KB (psi2, Qp = 64)
}
#define PSS_QG_SWITCH(QG, CALL, WIDEST)    \
    switch (QG) {                          \
        case 1: { CALL(1); } break;        \
        case 2: { CALL(2); } break;        \
        case 4: { CALL(4); } break;        \
        case 8: { CALL(8); } break;        \
        default: { CALL(WIDEST); } break;  \
    }
void launch_pss_psi1_grad(hipStream_t st, const double* rd1_, const double* Zp, const double* Ep, const double* G, long ldg,
                          PsiRank rk, long rows, long m, long mpad, int Qp, double var, double* Ppart, double* Zpart) {
    const double4* rd1 = (const double4*)rd1_;
    const int QG = Qp < PSS_DC ? Qp : PSS_DC;
    const dim3 grid((unsigned)((m + 15) / 16), (unsigned)((rows + PSI_GROWS - 1) / PSI_GROWS), (unsigned)(Qp / QG));
    const size_t lds = pss_grad_lds(Qp, QG, false);
#define PSS_CALL(N) hipLaunchKernelGGL((k_pss_psi1_grad<N>), grid, dim3(256), lds, st, rd1, Zp, Ep, G, ldg, rk, rows, m, mpad, Qp, var, Ppart, Zpart)
    PSS_QG_SWITCH(QG, PSS_CALL, PSS_DC)
#undef PSS_CALL
}
void launch_pss_psi2_grad(hipStream_t st, const double* rd2_, const double* w, const double* Zp, const double* Ep,
                          const double* ap, const double* dL, long ldd, long rows, long m, long mpad, int Qp, double var2,
                          double* Ppart, double* Zpart) {
    const double4* rd2 = (const double4*)rd2_;
    const int QG = Qp < PSS_DC2 ? Qp : PSS_DC2, OC = pss_oc(Qp);
    const dim3 grid((unsigned)((m + 15) / 16), (unsigned)((rows + PSI_GROWS - 1) / PSI_GROWS), (unsigned)(Qp / QG));
    const size_t lds = pss_grad_lds(Qp, QG, true);
#define PSS_CALL(N) hipLaunchKernelGGL((k_pss_psi2_grad<N>), grid, dim3(256), lds, st, rd2, w, Zp, Ep, ap, dL, ldd, rows, m, mpad, Qp, OC, var2, Ppart, Zpart)
    PSS_QG_SWITCH(QG, PSS_CALL, PSS_DC2)
#undef PSS_CALL
}

void launch_pss_e(hipStream_t st, const double* Zp, const double* a, long mpad, int Qp, double* Ep) {
    const long cnt = mpad * Qp;
    hipLaunchKernelGGL(k_pss_e, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, Zp, a, cnt, Qp, Ep);
}
void launch_pss_rows(hipStream_t st, const double* mu, const double* S, const double* gam, const double* a, long rows, int D,
                     int Qp, double* rd1, double* rd2) {
    hipLaunchKernelGGL(k_pss_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, mu, S, gam, a, rows, D, Qp, (double4*)rd1,
                       (double4*)rd2);
}
void launch_pss_psi1(hipStream_t st, const double* rd1, const double* Zp, const double* Ep, long rows, long m, long mpad, int Qp,
                     double var, double* out, long ldo) {
    hipLaunchKernelGGL(k_pss_psi1, dim3((unsigned)((rows + PSI_KT - 1) / PSI_KT), (unsigned)(mpad / PSI_KT)), dim3(256), 0, st,
                       (const double4*)rd1, Zp, Ep, rows, m, Qp, var, out, ldo);
}
void launch_pss_rowfinish(hipStream_t st, const double* P1s, const double* P2s, const double* S, const double* gam, const double* a,
                          long rows, int D, int Qp, double* dmu, double* dS, double* dgam, double* rowrec) {
    hipLaunchKernelGGL(k_pss_rowfinish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, P1s, P2s, S, gam, a, rows, D, Qp, dmu,
                       dS, dgam, rowrec);
}
// dZ += (Zs - a z Zk) of psi1 + 2 (Zs - a z Zk) of psi2 (dL_dpsi2 symmetric: both positions of z_m); lsum[q] += the inducing
// points' share of l_q dE/dl_q: a z^2 Zk of psi1 and a (Zq / 2 + 2 z^2 Zk) of psi2, summed over the inducing points in their order
void pss_finish_z(const double* zs1, const double* zs2, const double* a, const double* zp, long m, int D, int Qp, double* dZ,
                  double* lsum) {
    const int ZL = PSS_NZ * Qp;
    for (int q = 0; q < D; ++q) {
        double zl = 0.0;
        for (long i = 0; i < m; ++i) {
            const double z = zp[(size_t)i * Qp + q];
            const double *r1 = zs1 + (size_t)i * ZL, *r2 = zs2 + (size_t)i * ZL;
            if (dZ) dZ[i * D + q] += (r1[q] - a[q] * z * r1[Qp + q]) + 2.0 * (r2[q] - a[q] * z * r2[Qp + q]);
            zl += a[q] * (z * z * (r1[Qp + q] + 2.0 * r2[Qp + q]) + 0.5 * r2[2 * Qp + q]);
        }
        lsum[q] += zl;
    }
}

// ---- the stateless entry points ----------------------------------------------------------------------------------------
namespace {
// what both entry points validate and upload: the kernel's parameters, Z (padded) with its E, and the spike-and-slab inputs
struct PssInputs {
    PartSpec spec;
    int D = 0, Qp = 0;
    long N = 0, M = 0, mpad = 0;
    double var = 0.0;
    std::vector<double> a, zp;                                // Qp: 1 / l_q^2, 0 in the padding; mpad x Qp: Z zero padded
    DevBuf dA, dZp, dEp, dMu, dS, dGam, dW;
    int load(const char* where, double variance, const double* lengthscale, int ard, const double* Z, int64_t M_,
             const double* mu, const double* S, const double* gamma, int64_t N_, int D_, const double* weights) {
        if (!(lengthscale && Z && mu && S && gamma && M_ > 0 && N_ > 0 && D_ > 0)) PART_FAIL("%s: bad arguments", where);
        if (M_ > PSI_MMAX) PART_FAIL("%s: %lld inducing points; the psi-statistics kernels take at most %d", where, (long long)M_, PSI_MMAX);
        if (D_ > PSI_QMAX) PART_FAIL("%s: %d input dimensions; the psi-statistics kernels take at most %d", where, D_, PSI_QMAX);
        std::vector<double> th(1 + (size_t)(ard ? D_ : 1));
        th[0] = variance;
        for (size_t k = 1; k < th.size(); ++k) th[k] = lengthscale[k - 1];
        const mi355gp_part part{MI355GP_RBF, ard ? 1 : 0, 0, nullptr, th.data(), 0};
        if (int rc = parse_part(part, D_, 1u << MI355GP_RBF, where, &spec)) return rc;
        for (int64_t i = 0; i < N_ * D_; ++i) {
            if (!(S[i] > 0.0) || !std::isfinite(S[i]) || !std::isfinite(mu[i]))
                PART_FAIL("%s: input variance S[%lld][%lld] = %g (mean %g): every entry must be positive and finite", where,
                          (long long)(i / D_), (long long)(i % D_), S[i], mu[i]);
            if (!(gamma[i] > 0.0 && gamma[i] < 1.0))
                PART_FAIL("%s: slab probability gamma[%lld][%lld] = %g: every entry must lie strictly inside (0, 1)", where,
                          (long long)(i / D_), (long long)(i % D_), gamma[i]);
        }
        for (int64_t i = 0; i < M_ * D_; ++i)
            if (!std::isfinite(Z[i])) PART_FAIL("%s: Z[%lld][%lld] is not finite", where, (long long)(i / D_), (long long)(i % D_));
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
        zp.assign((size_t)mpad * Qp, 0.0);
        for (long i = 0; i < M; ++i)
            for (int q = 0; q < D; ++q) zp[(size_t)i * Qp + q] = Z[i * D + q];
        HIP_CHECK(dA.alloc(Qp));
        HIP_CHECK(dZp.alloc(zp.size()));
        HIP_CHECK(dEp.alloc(zp.size()));
        HIP_CHECK(dMu.alloc(N * D));
        HIP_CHECK(dS.alloc(N * D));
        HIP_CHECK(dGam.alloc(N * D));
        HIP_CHECK(hipMemcpy(dA, a.data(), sizeof(double) * Qp, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dZp, zp.data(), sizeof(double) * zp.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dMu, mu, sizeof(double) * N * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dS, S, sizeof(double) * N * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dGam, gamma, sizeof(double) * N * D, hipMemcpyHostToDevice));
        if (weights) {
            HIP_CHECK(dW.alloc(N));
            HIP_CHECK(hipMemcpy(dW, weights, sizeof(double) * N, hipMemcpyHostToDevice));
        }
        launch_pss_e(0, dZp, dA, mpad, Qp, dEp);
        return 0;
    }
};
// the per-row operands of one chunk (double4 records)
struct PssRows {
    DevBuf rd1, rd2;
    int alloc(long rows, int Qp) {
        HIP_CHECK(rd1.alloc(4 * rows * Qp));
        HIP_CHECK(rd2.alloc(4 * rows * Qp));
        return 0;
    }
    void fill(hipStream_t st, const PssInputs& in, long r0, long rc) {
        launch_pss_rows(st, in.dMu + r0 * in.D, in.dS + r0 * in.D, in.dGam + r0 * in.D, in.dA, rc, in.D, in.Qp, rd1, rd2);
    }
};
}  // namespace

extern "C" {

int mi355gp_ssrbf_psi(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                      const double* mu, const double* S, const double* gamma, int64_t N, int D, const double* weights,
                      double* psi1_out, double* psi2_out) {
    HIP_CHECK(hipSetDevice(device));
    PssInputs in;
    if (int rc = in.load("mi355gp_ssrbf_psi", variance, lengthscale, ard, Z, M, mu, S, gamma, N, D, weights)) return rc;
    hipStream_t st = 0;
    const long chunk = N < PSI_CHUNK ? N : PSI_CHUNK, ld = round_up(M, PSI_T2);
    PssRows rw;
    if (int rc = rw.alloc(chunk, in.Qp)) return rc;
    DevBuf d1, part, d2;
    if (psi1_out) HIP_CHECK(d1.alloc(chunk * M));
    if (psi2_out) {
        HIP_CHECK(part.alloc((size_t)psi2_nsplit(chunk, M) * ld * ld));
        HIP_CHECK(d2.alloc(M * M));
    }
    int nch = 0;
    for (long r0 = 0; r0 < N; r0 += PSI_CHUNK, ++nch) {      // chunks in row order
        const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
        rw.fill(st, in, r0, rc);
        if (psi1_out) {
            launch_pss_psi1(st, rw.rd1, in.dZp, in.dEp, rc, (long)M, in.mpad, in.Qp, variance, d1, (long)M);
            HIP_CHECK(hipMemcpy(psi1_out + r0 * M, d1, sizeof(double) * rc * M, hipMemcpyDeviceToHost));
        }
        if (psi2_out) {
            const int ns = launch_pss_psi2(st, rw.rd2, in.dW ? in.dW + r0 : nullptr, in.dZp, in.dEp, in.dA, rc,
                                           (long)M, in.Qp, variance * variance, ld, part);
            launch_psi2_combine(st, part, ld, (long)M, ns, nch > 0, d2, (long)M);
        }
    }
    if (psi2_out) HIP_CHECK(hipMemcpy(psi2_out, d2, sizeof(double) * M * M, hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    return 0;
}

int mi355gp_ssrbf_psi_grad(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                           const double* mu, const double* S, const double* gamma, int64_t N, int D, const double* weights,
                           const double* dL_dpsi0, const double* dL_dpsi1, const double* dL_dpsi2, double* dvar_out,
                           double* dl_out, double* dZ_out, double* dmu_out, double* dS_out, double* dgamma_out) {
    ARG_CHECK(dvar_out && dl_out && dZ_out && dmu_out && dS_out && dgamma_out, "mi355gp_ssrbf_psi_grad: NULL output");
    HIP_CHECK(hipSetDevice(device));
    PssInputs in;
    if (int rc = in.load("mi355gp_ssrbf_psi_grad", variance, lengthscale, ard, Z, M, mu, S, gamma, N, D, weights)) return rc;
    hipStream_t st = 0;
    const int Qp = in.Qp, RL = 1 + 4 * Qp, ZL = PSS_NZ * Qp;
    const long chunk = N < PSI_CHUNK ? N : PSI_CHUNK, mpad = in.mpad, mt = (M + 15) / 16;
    const long nzb = (chunk + PSI_GROWS - 1) / PSI_GROWS;
    PssRows rw;
    if (int rc = rw.alloc(chunk, Qp)) return rc;
    DevBuf dG, dL2, Ppart, P1s, P2s, Zpart, Zs1, Zs2, dMuO, dSO, dGO, rowrec, rec;
    std::vector<double> zs1((size_t)mpad * ZL, 0.0), zs2((size_t)mpad * ZL, 0.0);
    std::vector<double> sums((size_t)(1 + Qp), 0.0), csum((size_t)(1 + Qp));
    HIP_CHECK(Ppart.alloc((size_t)mt * chunk * RL));
    HIP_CHECK(P1s.alloc((size_t)chunk * RL));
    HIP_CHECK(P2s.alloc((size_t)chunk * RL));
    HIP_CHECK(Zpart.alloc((size_t)nzb * mpad * ZL));
    HIP_CHECK(hipMemset(Zpart, 0, sizeof(double) * nzb * mpad * ZL));       // the kernels write rows < round_up(M, 16) only
    HIP_CHECK(Zs1.alloc((size_t)mpad * ZL));
    HIP_CHECK(Zs2.alloc((size_t)mpad * ZL));
    HIP_CHECK(dMuO.alloc(chunk * D));
    HIP_CHECK(dSO.alloc(chunk * D));
    HIP_CHECK(dGO.alloc(chunk * D));
    HIP_CHECK(rowrec.alloc((size_t)chunk * (1 + Qp)));
    HIP_CHECK(rec.alloc(1 + Qp));
    if (dL_dpsi1) HIP_CHECK(dG.alloc(chunk * M));
    if (dL_dpsi2) {                                            // symmetrised on the way in (ssrbf_psi_comp.py assumes it)
        std::vector<double> sym((size_t)M * M);
        for (long i = 0; i < M; ++i)
            for (long j = 0; j < M; ++j) sym[(size_t)i * M + j] = 0.5 * (dL_dpsi2[i * M + j] + dL_dpsi2[j * M + i]);
        HIP_CHECK(dL2.alloc(M * M));
        HIP_CHECK(hipMemcpy(dL2, sym.data(), sizeof(double) * M * M, hipMemcpyHostToDevice));
    }
    int nch = 0;
    for (long r0 = 0; r0 < N; r0 += PSI_CHUNK, ++nch) {
        const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
        const int nb = (int)((rc + PSI_GROWS - 1) / PSI_GROWS);
        rw.fill(st, in, r0, rc);
        if (dL_dpsi1) {
            HIP_CHECK(hipMemcpy(dG, dL_dpsi1 + r0 * M, sizeof(double) * rc * M, hipMemcpyHostToDevice));
            launch_pss_psi1_grad(st, rw.rd1, in.dZp, in.dEp, dG, (long)M, PsiRank{nullptr, nullptr, 0, 0.0}, rc, (long)M, mpad, Qp,
                                 variance, Ppart, Zpart);
            launch_sum_splits(st, Ppart, rc * RL, (int)mt, 0, P1s);
            launch_sum_splits(st, Zpart, mpad * ZL, nb, nch > 0, Zs1);
        }
        if (dL_dpsi2) {
            launch_pss_psi2_grad(st, rw.rd2, in.dW ? in.dW + r0 : nullptr, in.dZp, in.dEp, in.dA, dL2, (long)M, rc,
                                 (long)M, mpad, Qp, variance * variance, Ppart, Zpart);
            launch_sum_splits(st, Ppart, rc * RL, (int)mt, 0, P2s);
            launch_sum_splits(st, Zpart, mpad * ZL, nb, nch > 0, Zs2);
        }
        launch_pss_rowfinish(st, dL_dpsi1 ? (const double*)P1s.p : nullptr, dL_dpsi2 ? (const double*)P2s.p : nullptr, in.dS + r0 * D,
                             in.dGam + r0 * D, in.dA, rc, D, Qp, dMuO, dSO, dGO, rowrec);
        launch_reduce_partials(st, rowrec, (int)rc, 1 + Qp, rec);
        HIP_CHECK(hipMemcpy(dmu_out + r0 * D, dMuO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(dS_out + r0 * D, dSO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(dgamma_out + r0 * D, dGO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(csum.data(), rec, sizeof(double) * (1 + Qp), hipMemcpyDeviceToHost));
        for (int k = 0; k <= Qp; ++k) sums[(size_t)k] += csum[(size_t)k];                          // chunks in row order
    }
    if (dL_dpsi1) HIP_CHECK(hipMemcpy(zs1.data(), Zs1, sizeof(double) * zs1.size(), hipMemcpyDeviceToHost));
    if (dL_dpsi2) HIP_CHECK(hipMemcpy(zs2.data(), Zs2, sizeof(double) * zs2.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    for (int64_t i = 0; i < M * D; ++i) dZ_out[i] = 0.0;
    pss_finish_z(zs1.data(), zs2.data(), in.a.data(), in.zp.data(), (long)M, D, Qp, dZ_out, sums.data() + 1);
    const int groups = (D + 31) / 32;
    std::vector<double> recs((size_t)groups * GP_STRIDE, 0.0), th(in.spec.theta.size());
    double v0 = sums[0];
    if (dL_dpsi0)
        for (int64_t i = 0; i < N; ++i) v0 += dL_dpsi0[i] * variance;                              // psi0 = variance
    recs[0] = v0;
    for (int q = 0; q < D; ++q) {
        const double lq = sums[(size_t)(1 + q)];
        recs[(size_t)(q / 32) * GP_STRIDE + 2 + (q % 32)] = -lq;
        recs[1] -= lq;
    }
    part_dtheta(in.spec, recs.data(), nullptr, th.data());
    *dvar_out = th[0];
    for (size_t k = 1; k < th.size(); ++k) dl_out[k - 1] = th[k];
    return 0;
}

}  // extern "C"
