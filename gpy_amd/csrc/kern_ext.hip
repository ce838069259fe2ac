// kern_ext.hip -- the ext family: the kinds that are a function of a scaled distance other than the stationary ones (RatQuad,
// Cosine, Sinc, ExpQuadCosine) and StdPeriodic with its dK/dx pass.  One K-build kernel and one gradient kernel, templates on
// the kind, around the skeleton of kern_tile.h; kern.hip's dispatch reaches them through launch_kbuild_ext / launch_grad_ext
// (declared in kern_tile.h).  A file of its own for the build's sake: ten instantiations of each kernel.
#include <cstdint>
#include <cstdlib>

#include "../../include/mi355gp.h"
#include "internal.h"
#include "kern_tile.h"

// ------------------------------------------------------------------------------------------------
// RatQuad (kind 6, stationary.py:747-802) and StdPeriodic (kind 7, standard_periodic.py:15-580).
// Their own kernels (templates on the kind) around the shared skeleton: the accumulate step and the element are what differs.
//   RatQuad:     K = var exp(-a log1p(r^2 / 2)),  dK/dr / r = -a K / (1 + r^2 / 2),  dK/da = -K log1p(r^2 / 2)
//                (inputs scaled by 1 / l as for the other stationary kinds)
//   StdPeriodic: K = var exp(-1/2 sum_q (sin(Delta_q) / l_q)^2),  Delta_q = pi (x_iq - x_jq) / T_q
//                (inputs staged UNSCALED: Delta is formed from the difference of the raw coordinates, so calendar-year
//                inputs keep their precision; pi / T_q and 1 / l_q are applied per dimension in the pair loop)

__device__ __forceinline__ void ratquad_all(double var, double a, double r2, double& k, double& dk_or, double& dk_a) {
    const double h = 0.5 * r2;
    const double lg = log1p(h);
    k = var * exp(-a * lg);
    dk_or = -a * k / (1.0 + h);
    dk_a = -k * lg;
}

// Cosine (kind 12, stationary.py:664-680), Sinc (kind 13, :717-743) and ExpQuadCosine (kind 14, :682-713): functions of the
// scaled distance r = sqrt(s) alone, in the kernels of RatQuad (inputs scaled by 1 / l).  Each helper returns K and (dK/dr) / r
// from ONE sincos evaluation; (dK/dr) / r is 0 at r = 0, the reference's _inv_dist convention (:225-232).  The arguments of
// Sinc and ExpQuadCosine are multiples of pi: sincospi reduces 2 r and 2 r / T exactly instead of a product with a rounded pi.
//   Cosine:        K = var cos r,                           dK/dr = -var sin r
//   Sinc:          K = var sinc(2 r) = var sin(2 pi r) / (2 pi r),  dK/dr = var (cos(2 pi r) - sinc(2 r)) / r
//   ExpQuadCosine: K = var E cos(2 pi r / T), E = exp(-2 pi^2 r^2),  dK/dr = -4 pi^2 r K - var (2 pi / T) E sin(2 pi r / T),
//                  dK/dT = var (2 pi r / T^2) E sin(2 pi r / T)     (kp.power carries T)
#define OSC_2PI2 (2.0 * M_PI * M_PI)
#define OSC_4PI2 (4.0 * M_PI * M_PI)

__device__ __forceinline__ void cosine_all(double var, double s, double& k, double& dk_or) {
    const double r = sqrt(s);
    double sn, cs;
    sincos(r, &sn, &cs);
    k = var * cs;
    dk_or = (r > 0.0) ? -var * sn / r : 0.0;
}

// cos t - sin t / t = sum_{k >= 1} (-1)^k 2k / (2k + 1)! u^k in u = t^2 = 4 pi^2 s.  Below u = 1 the difference of the two
// rounded values would cancel (the reference switches to its leading term -u / 3 below r = 1e-5, :733-743); ten terms leave a
// truncation of 22 / 23! < 1e-21 there.
__device__ __forceinline__ double sinc_diff_series(double u) {
    double p = 20.0 / 51090942171709440000.0;                  // 20 / 21!
    p = fma(p, u, -18.0 / 121645100408832000.0);               // 18 / 19!
    p = fma(p, u, 16.0 / 355687428096000.0);                   // 16 / 17!
    p = fma(p, u, -14.0 / 1307674368000.0);                    // 14 / 15!
    p = fma(p, u, 12.0 / 6227020800.0);                        // 12 / 13!
    p = fma(p, u, -10.0 / 39916800.0);                         // 10 / 11!
    p = fma(p, u, 8.0 / 362880.0);                             // 8 / 9!
    p = fma(p, u, -6.0 / 5040.0);                              // 6 / 7!
    p = fma(p, u, 4.0 / 120.0);                                // 4 / 5!
    p = fma(p, u, -2.0 / 6.0);                                 // 2 / 3!
    return p;                                                  // (cos t - sin t / t) / u
}

__device__ __forceinline__ void sinc_all(double var, double s, double& k, double& dk_or) {
    const double x = 2.0 * sqrt(s), u = OSC_4PI2 * s;
    double sn, cs;
    sincospi(x, &sn, &cs);
    const double snc = (x > 0.0) ? sn / (M_PI * x) : 1.0;
    k = var * snc;
    // (dK/dr) / r = var (cos t - sinc) / r^2 = 4 pi^2 var (cos t - sinc) / u
    if (u < 1.0) dk_or = (s > 0.0) ? OSC_4PI2 * var * sinc_diff_series(u) : 0.0;
    else dk_or = var * (cs - snc) / s;
}

__device__ __forceinline__ void eqc_all(double var, double T, double s, double& k, double& dk_or, double& dk_T) {
    const double r = sqrt(s), e = var * exp(-OSC_2PI2 * s);
    double sn, cs;
    sincospi(2.0 * r / T, &sn, &cs);
    const double w = 2.0 * M_PI / T * e * sn;                  // var (2 pi / T) E sin(2 pi r / T)
    k = e * cs;
    dk_or = (r > 0.0) ? -OSC_4PI2 * k - w / r : 0.0;
    dk_T = w * r / T;
}

// K, (dK/dr) / r and the derivative by the kind's scalar parameter (RatQuad: power, ExpQuadCosine: period; 0 otherwise)
template <int KIND>
__device__ __forceinline__ void ext_all(const KernParams& kp, double s, double& k, double& dk_or, double& dk_p) {
    if (KIND == MI355GP_RATQUAD) {
        ratquad_all(kp.variance, kp.power, s, k, dk_or, dk_p);
    } else if (KIND == MI355GP_COSINE) {
        cosine_all(kp.variance, s, k, dk_or);
        dk_p = 0.0;
    } else if (KIND == MI355GP_SINC) {
        sinc_all(kp.variance, s, k, dk_or);
        dk_p = 0.0;
    } else {
        eqc_all(kp.variance, kp.power, s, k, dk_or, dk_p);
    }
}

// s[a][b] += sum_q (sin(pi / T_q (xi[q][ty*4+a] - xj[q][tx*4+b])) / l_q)^2 over the staged dimensions q0 .. q0 + qc
__device__ __forceinline__ void accum_per(const double* si, const double* sj, const double* __restrict__ pw, int D, int q0, int qc,
                                          int ty, int tx, double (&s)[4][4]) {
    for (int q = 0; q < qc; ++q) {
        const double pt = pw[q0 + q], il = pw[D + q0 + q];
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double sn = sin((xi[a] - xj[b]) * pt) * il;
                s[a][b] = fma(sn, sn, s[a][b]);
            }
    }
}

template <int KIND>
__device__ __forceinline__ void accum_ext(const double* si, const double* sj, const KernParams& kp, int q0, int qc, int ty, int tx,
                                          double (&s)[4][4]) {
    if (KIND != MI355GP_STDPERIODIC) accum_r2(si, sj, qc, ty, tx, s);
    else accum_per(si, sj, kp.pw, kp.D, q0, qc, ty, tx, s);
}

template <int KIND>
__device__ __forceinline__ double ext_k(const KernParams& kp, double s) {
    if (KIND == MI355GP_RATQUAD) return kp.variance * exp(-kp.power * log1p(0.5 * s));
    if (KIND == MI355GP_COSINE) return kp.variance * cos(sqrt(s));
    if (KIND == MI355GP_SINC) {
        const double x = 2.0 * sqrt(s);
        return kp.variance * ((x > 0.0) ? sinpi(x) / (M_PI * x) : 1.0);
    }
    if (KIND == MI355GP_EXPQUADCOSINE) return kp.variance * exp(-OSC_2PI2 * s) * cospi(2.0 * sqrt(s) / kp.power);
    return kp.variance * exp(-0.5 * s);
}

// Covariance assembly for these kinds: no White-like diagonal in any.
template <bool SYM, int KIND>
__global__ __launch_bounds__(256) void k_kbuild_ext(KbuildArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double s[4][4];
    zero_tile(s);
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC)
            accum_ext<KIND>(si, sj, A.kp, q0, stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t), ty, tx, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) v[b] = ext_k<KIND>(A.kp, s[a][b]);
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient pass of k_grad for these kinds, one launch per group of 32 dimensions (q_off).  Record A [GP_STRIDE] per block:
//   [0] sum g K, RatQuad [1] sum g dK/dr r (isotropic) or [2 + q] sum g (dK/dr / r) (x~_iq - x~_jq)^2 (ARD)
//   (Cosine, Sinc and ExpQuadCosine as RatQuad; record B [0] of ExpQuadCosine: sum g dK/dperiod, none for the other two),
//   StdPeriodic [2 + q] sum g K sin(D_q) cos(D_q) D_q (period);
// record B, which follows every group's record A (at A.partials + groups * blocks * GP_STRIDE): RatQuad [0] sum g dK/dpower, StdPeriodic [2 + q] sum g K sin^2(D_q) (lengthscale).
// StdPeriodic always reduces per dimension; the host applies 1 / (T_q l_q^2), 1 / l_q^3 and sums the isotropic cases.
template <bool FUSED, int KIND>
__global__ __launch_bounds__(256) void k_grad_ext(GradArgs A) {
    constexpr bool PER = (KIND == MI355GP_STDPERIODIC);
    constexpr bool SCALAR = (KIND == MI355GP_RATQUAD || KIND == MI355GP_EXPQUADCOSINE);   // a scalar parameter: record B [0]
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const KernParams& kp = A.kp;
    double a_var = 0.0, a_iso = 0.0, a_pow = 0.0;
    double a1[KDC], a2[KDC];   // a2: StdPeriodic alone
#pragma unroll
    for (int q = 0; q < KDC; ++q) a1[q] = a2[q] = 0.0;
    const int qcnt = grad_qcnt(PER || kp.ard, kp.D, A.q_off);
    const double sc = grad_aa_scale<FUSED>(A.aa_scale);

    for (long tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, A.ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double s[4][4];
        zero_tile(s);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC)
            accum_ext<KIND>(si, sj, kp, q0, stage_chunk(A, q0, i0, j0, si, sj, t), ty, tx, s);
        double gw[4][4];   // functions of r: g dK/dr / r;  StdPeriodic: g K
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                const double g = grad_weight<FUSED, true>(A, i, j, sc);
                if (PER) {
                    const double k = kp.variance * exp(-0.5 * s[a][b]);
                    a_var = fma(g, k, a_var);
                    gw[a][b] = g * k;
                } else {
                    double k, dk_or, dk_a;
                    ext_all<KIND>(kp, s[a][b], k, dk_or, dk_a);
                    a_var = fma(g, k, a_var);
                    if (SCALAR) a_pow = fma(g, dk_a, a_pow);
                    if (!kp.ard) a_iso = fma(g, dk_or * s[a][b], a_iso);
                    gw[a][b] = g * dk_or;
                }
            }
        }
        // functions of r: H = dL_dK (dK/dr) / r as in k_grad (0 at r = 0); StdPeriodic has its own dK/dx pass (k_periodic_gradx)
        if (!PER && !FUSED && A.Hout) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    store_h<true>(A.Hout, A.ldh, i0 + ty * 4 + a, j0 + tx * 4 + b, A.n, A.m, s[a][b], gw[a][b]);
        }
        if (qcnt > 0) {
            restage(A, last_q0, qcnt, i0, j0, si, sj, t);
#pragma unroll
            for (int q = 0; q < KDC; ++q) {   // (for_each_dim spelt out: through the lambda StdPeriodic takes 56 more registers)
                if (q < qcnt) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    if (PER) {
                        const double pt = kp.pw[A.q_off + q];
                        double s1 = 0.0, s2 = 0.0;
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const double dl = (xi[a] - xj[b]) * pt;
                                double sn, cs;
                                sincos(dl, &sn, &cs);
                                s1 = fma(gw[a][b], sn * cs * dl, s1);
                                s2 = fma(gw[a][b], sn * sn, s2);
                            }
                        a1[q] += s1;
                        a2[q] += s2;
                    } else {
                        double s1 = 0.0;
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const double d = xi[a] - xj[b];
                                s1 = fma(gw[a][b], d * d, s1);
                            }
                        a1[q] += s1;
                    }
                }
            }
        }
    }
    double* outA = A.partials + (long)blockIdx.x * GP_STRIDE;
    double* outB = outA + (long)((kp.D + KDC - 1) / KDC) * gridDim.x * GP_STRIDE;
    grad_put(outA, 0, t, a_var);
    if (!PER) {
        if (SCALAR) grad_put(outB, 0, t, a_pow);
        if (!kp.ard) grad_put(outA, 1, t, a_iso);
    }
    if (PER) grad_put_dims(outA, outB, qcnt, t, a1, a2);
    else grad_put_dims(outA, qcnt, t, a1);
}

// One launch per group of 32 dimensions where the kind reduces per dimension; the second records follow every group's first.
template <int KIND>
static void grad_ext(hipStream_t st, bool fused, int nb, const GradArgs& A) {
    launch_grad_kernel(st, fused, nb, A, k_grad_ext<true, KIND>, k_grad_ext<false, KIND>);
}
void launch_grad_ext(hipStream_t st, bool fused, const GradArgs& A) {
    const int nb = pick_grad_blocks(A.ntiles);
    for_each_group(A.kp.kind == MI355GP_STDPERIODIC || A.kp.ard, nb, A, [&](const GradArgs& g) {
        switch (g.kp.kind) {
        case MI355GP_STDPERIODIC: grad_ext<MI355GP_STDPERIODIC>(st, fused, nb, g); break;
        case MI355GP_COSINE: grad_ext<MI355GP_COSINE>(st, fused, nb, g); break;
        case MI355GP_SINC: grad_ext<MI355GP_SINC>(st, fused, nb, g); break;
        case MI355GP_EXPQUADCOSINE: grad_ext<MI355GP_EXPQUADCOSINE>(st, fused, nb, g); break;
        default: grad_ext<MI355GP_RATQUAD>(st, fused, nb, g); break;
        }
    });
}

// StdPeriodic dK/dx as a row reduction (see internal.h).  Block = 64 rows x 4 column lanes; the block walks every 64-column
// tile, the covariance of each pair is formed over all dimensions first (chunks of 32), then the dimensions of the group
// q_off .. q_off + 31 are accumulated.  The four lanes of a row are combined in fixed order: bit reproducible.
__global__ __launch_bounds__(256) void k_periodic_gradx(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                        const double* __restrict__ Xt2, long ld2, long m,
                                                        const double* __restrict__ W, long ldw, int wt, int q_off,
                                                        double* __restrict__ out) {
    __shared__ double si[KDC * KT];
    __shared__ double sj[KDC * KT];
    __shared__ double red[4][KT];
    const int t = threadIdx.x, r = t & 63, l = t >> 6;
    const long i0 = (long)blockIdx.x * KT, i = i0 + r;
    const int qcnt = (kp.D - q_off < KDC) ? (kp.D - q_off) : KDC;
    const double* __restrict__ pt = kp.pw;
    const double* __restrict__ il = kp.pw + kp.D;
    double acc[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) acc[q] = 0.0;
    for (long j0 = 0; j0 < m; j0 += KT) {
        double s[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) s[c] = 0.0;
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; q0 += KDC) {
            const int qc = (kp.D - q0 < KDC) ? (kp.D - q0) : KDC;
            __syncthreads();
            stage_x(Xt1, ld1, i0, q0, qc, si, t);
            stage_x(Xt2, ld2, j0, q0, qc, sj, t);
            __syncthreads();
            for (int q = 0; q < qc; ++q) {
                const double xi = si[q * KT + r], p = pt[q0 + q], w = il[q0 + q];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const double sn = sin((xi - sj[q * KT + 4 * c + l]) * p) * w;
                    s[c] = fma(sn, sn, s[c]);
                }
            }
            last_q0 = q0;
        }
        // weights W(i, j) K(i, j)
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const long j = j0 + 4 * c + l;
            double wk = 0.0;
            if (i < n && j < m) wk = (wt ? W[j * ldw + i] : W[i * ldw + j]) * kp.variance * exp(-0.5 * s[c]);
            s[c] = wk;
        }
        if (last_q0 != q_off) {
            __syncthreads();
            stage_x(Xt1, ld1, i0, q_off, qcnt, si, t);
            stage_x(Xt2, ld2, j0, q_off, qcnt, sj, t);
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < KDC; ++q) {
            if (q < qcnt) {
                const double xi = si[q * KT + r], p = pt[q_off + q];
                double a = 0.0;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    double sn, cs;
                    sincos((xi - sj[q * KT + 4 * c + l]) * p, &sn, &cs);
                    a = fma(s[c], 2.0 * sn * cs, a);
                }
                acc[q] += a;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KDC; ++q) {
        if (q < qcnt) {
            __syncthreads();
            red[l][r] = acc[q];
            __syncthreads();
            if (l == 0 && i < n) out[i * kp.D + q_off + q] = (red[0][r] + red[1][r]) + (red[2][r] + red[3][r]);
        }
    }
}

void launch_periodic_gradx(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                           long m, const double* W, long ldw, int wt, double* out) {
    const unsigned nbr = (unsigned)((n + KT - 1) / KT);
    for (int q_off = 0; q_off < kp.D; q_off += KDC)
        hipLaunchKernelGGL(k_periodic_gradx, dim3(nbr), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, W, ldw, wt, q_off, out);
}

template <bool SYM>
static void kbuild_ext(hipStream_t st, long nblocks, const KbuildArgs& A) {
    const dim3 g((unsigned)nblocks), b(256);
    switch (A.kp.kind) {
    case MI355GP_STDPERIODIC: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_STDPERIODIC>), g, b, 0, st, A); break;
    case MI355GP_COSINE: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_COSINE>), g, b, 0, st, A); break;
    case MI355GP_SINC: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_SINC>), g, b, 0, st, A); break;
    case MI355GP_EXPQUADCOSINE: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_EXPQUADCOSINE>), g, b, 0, st, A); break;
    default: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_RATQUAD>), g, b, 0, st, A); break;
    }
}
void launch_kbuild_ext(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A) {
    if (sym) kbuild_ext<true>(st, nblocks, A);
    else kbuild_ext<false>(st, nblocks, A);
}
