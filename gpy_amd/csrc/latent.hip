// latent.hip -- the gradient phase of an exact-GP evaluation whose inputs are parameters (GPLVM, GPy/models/gplvm.py): ONE pass
// over the resident W = Ky^-1 and alpha gives dL/dX and the kernel-parameter sums of a stationary part together
// (stationary.py:245-252, 330-358).  With x~ = x / l, il_q = 1 / l_q (0 outside active_dims):
//   g_ij = 0.5 (alpha_i . alpha_j - Dy W_ij),   h_ij = g_ij (dK/dr) / r   (0 where r = 0: stationary.py:231-232),
//   dX[i, q] = 2 il_q sum_j h_ij (x~_iq - x~_jq)
// and the record of launch_grad_fused: [0] sum g K, [1] sum h r^2 (isotropic) or [2 + q] sum h (x~_iq - x~_jq)^2 (ARD), RatQuad's
// second record [0] sum g dK/dpower.  No N x N array is written.
//
// k_latent_grad<KIND>: a workgroup of four waves owns the 128-row block I and a strip of 64-column steps J, walked in ascending J
// over the FULL square (W of the upper steps is read from the mirrored lower tile), so every output row has one owner: wave w
// keeps rows 32 w .. 32 w + 31 of [S_i | T_iq] in accumulators over the whole walk; no symmetric scatter, no atomics.
//   1. alpha alpha^T on v_mfma_f64_16x16x4_f64: the alpha_I and alpha_J slabs stream over Dy through LDS in k-slabs of 16 (the
//      remainder zero-filled), operands ordered so that the accumulators hold the tile TRANSPOSED (rows J, columns I).
//   2. element-wise in the accumulator layout (lane l, register r: row j = (l >> 4) + 4 r, column i = l & 15): W straight into
//      that layout, r^2 = sum_q (x~_iq - x~_jq)^2 from the x~ slabs in LDS, the kind's K and (dK/dr) / r, the theta sums.
//   3. register chaining: the accumulator block of h IS the A operand of the transposed product with k = (l >> 4) + 4 r (common.h),
//      the B fragments [x~_J - c_I | 1] come from LDS with the same k order, and the product lands on rows I:
//      S_i = sum_j h_ij, T_iq = sum_j h_ij (x~_jq - c_q), c_I = the first point of block I.  dX-sum = (x~_iq - c_q) S_i - T_iq.
// Strips exist to fill the CUs; their partials are summed in strip order by k_latent_sum, the theta sums and the ARD sums
//   sum_ij h_ij (x~_iq - x~_jq)^2 = sum_i (x~_iq - x~_0q) 2 G_iq,  G_iq = sum_j h_ij (x~_iq - x~_jq)   (h symmetric, sum_i G_iq = 0)
// by k_latent_rec: every sum has a fixed order, two runs give the same bytes.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi355gp_debug_latent.h"
#include "../../include/mi355gp_latent.h"
#include "ctx.h"
#include "kern_tile.h"

#define LT 128                 // rows of a block
#define LTJ 64                 // columns of a step
#define LJS 66                 // row stride of the staged x~_J slab (2 * odd, as LXS)
#define LKS 16                 // doubles of alpha per row in one k-slab
#define LAS 17                 // row stride of a staged alpha slab
#define LXS 130                // row stride of a staged x~ slab (2 * odd: lanes that differ in q fall on different banks)
#define LQ 32                  // most input dimensions
#define LQB 3                  // 16-column blocks of [x~ (<= 32) | 1]
#define LATENT_LDS (sizeof(double) * (LQ * LXS + 16 * LQB * LJS + (LT + LTJ) * LAS))

struct LatentArgs {
    KernParams kp;
    const double* Xt;          // scaled, dimension-major inputs [D][ldx], zero in [n, ldx)
    long ldx, n;
    const double* W;           // Ky^-1, lower 128-tiles valid, ld = ldw >= n rounded up to 128
    long ldw;
    const double* alpha;       // n x Dy
    int Dy, nt, ntj, S;        // nt row blocks, ntj column steps in S strips
    double* part;              // [S][n][D]: G_iq of strip s
    double* tpart;             // [nt * S][4]: sum g K, sum h r^2, sum g dK/dpower
};

template <int KIND>
__device__ __forceinline__ void latent_cov(const KernParams& kp, double r2, double& k, double& dk_or, double& dk_p) {
    if (KIND == MI355GP_RATQUAD) {
        ratquad_all(kp.variance, kp.power, r2, k, dk_or, dk_p);
    } else {
        const CovVal c = cov_all(KIND, kp.variance, r2, false);
        k = c.k;
        dk_or = c.dk_or;
        dk_p = 0.0;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_latent_grad(LatentArgs A) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* xI = smem;                         // [LQ][LXS]
    double* xJ = xI + LQ * LXS;                // [16 LQB][LJS]: rows q < D x~_J, row D ones, zeros up to qpad
    double* aI = xJ + 16 * LQB * LJS;          // [LT][LAS]
    double* aJ = aI + LT * LAS;                // [LTJ][LAS]
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lr = l & 15, lk = l >> 4;
    const int D = A.kp.D, nqb = (D + 16) >> 4, qpad = nqb << 4;
    const long n = A.n, i0 = (long)blockIdx.x * LT;
    const int s = blockIdx.y;
    const int jt0 = (int)((long)s * A.ntj / A.S), jt1 = (int)((long)(s + 1) * A.ntj / A.S);
    const double dy = (double)A.Dy;

    for (int idx = t; idx < D * LT; idx += 256) {
        const int q = idx >> 7, ii = idx & (LT - 1);
        xI[q * LXS + ii] = A.Xt[(long)q * A.ldx + i0 + ii];
    }
    double cq[LQB];                            // the centre of the lane's columns q = 16 qb + lr (0 for the ones column and the padding)
#pragma unroll
    for (int qb = 0; qb < LQB; ++qb) cq[qb] = (16 * qb + lr < D) ? A.Xt[(long)(16 * qb + lr) * A.ldx + i0] : 0.0;

    d4 out[2][LQB];
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int qb = 0; qb < LQB; ++qb) out[ib][qb] = (d4){0.0, 0.0, 0.0, 0.0};
    double a_var = 0.0, a_iso = 0.0, a_pow = 0.0;

    for (int jt = jt0; jt < jt1; ++jt) {
        const long j0 = (long)jt * LTJ;
        __syncthreads();                       // the previous step's readers of xJ are done (and xI is there)
        for (int idx = t; idx < qpad * LTJ; idx += 256) {
            const int q = idx >> 6, jj = idx & (LTJ - 1);
            xJ[q * LJS + jj] = (q < D) ? A.Xt[(long)q * A.ldx + j0 + jj] : (q == D ? 1.0 : 0.0);
        }
        // 1. T (rows J, columns I) = alpha_J alpha_I^T
        d4 T[2][LTJ / 16];
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int jb = 0; jb < LTJ / 16; ++jb) T[ib][jb] = (d4){0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < A.Dy; d0 += LKS) {
            __syncthreads();
            for (int idx = t; idx < LT * LKS; idx += 256) {
                const int row = idx >> 4, k = idx & (LKS - 1);
                const bool ink = d0 + k < A.Dy;
                aI[row * LAS + k] = (ink && i0 + row < n) ? A.alpha[(i0 + row) * A.Dy + d0 + k] : 0.0;
                if (row < LTJ) aJ[row * LAS + k] = (ink && j0 + row < n) ? A.alpha[(j0 + row) * A.Dy + d0 + k] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int k = lk + 4 * ks;
                const double b0 = aI[(w * 32 + lr) * LAS + k], b1 = aI[(w * 32 + 16 + lr) * LAS + k];
#pragma unroll
                for (int jb = 0; jb < LTJ / 16; ++jb) {
                    const double a = aJ[(jb * 16 + lr) * LAS + k];
                    T[0][jb] = mfma_f64(a, b0, T[0][jb]);
                    T[1][jb] = mfma_f64(a, b1, T[1][jb]);
                }
            }
        }
        __syncthreads();                       // xJ is there (Dy >= 1: at least one barrier pair above, this one for the slab-free reader)
        // 2. + 3. per 16 x 16 block: h in the accumulator layout, then out (rows I) += h^T [x~_J - c | 1]
#pragma unroll
        for (int ib = 0; ib < 2; ++ib) {
            const int li = w * 32 + ib * 16 + lr;
            const long gi = i0 + li;
#pragma unroll
            for (int jb = 0; jb < LTJ / 16; ++jb) {
                const int lj = jb * 16 + lk;   // + 4 r
                double r2[4] = {0.0, 0.0, 0.0, 0.0};
                for (int q = 0; q < D; ++q) {
                    const double xi = xI[q * LXS + li];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double d = xi - xJ[q * LJS + lj + 4 * r];
                        r2[r] = fma(d, d, r2[r]);
                    }
                }
                double h[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long gj = j0 + lj + 4 * r;
                    double g = 0.0;
                    if (gi < n && gj < n) {
                        const long hi = gi > gj ? gi : gj, lo = gi > gj ? gj : gi;
                        g = 0.5 * (T[ib][jb][r] - dy * A.W[hi * A.ldw + lo]);
                    }
                    double k, dk_or, dk_p;
                    latent_cov<KIND>(A.kp, r2[r], k, dk_or, dk_p);
                    a_var = fma(g, k, a_var);
                    if (KIND == MI355GP_RATQUAD) a_pow = fma(g, dk_p, a_pow);
                    h[r] = (r2[r] == 0.0) ? 0.0 : g * dk_or;
                    a_iso = fma(h[r], r2[r], a_iso);
                }
#pragma unroll
                for (int qb = 0; qb < LQB; ++qb)
                    if (qb < nqb) {
                        const double* xb = xJ + (16 * qb + lr) * LJS + lj;
#pragma unroll
                        for (int r = 0; r < 4; ++r) out[ib][qb] = mfma_f64(h[r], xb[4 * r] - cq[qb], out[ib][qb]);
                    }
                __builtin_amdgcn_sched_barrier(0);             // block by block: the scheduler does not pile the blocks' loads up
            }
        }
    }
    // G_iq = (x~_iq - c_q) S_i - T_iq: register r of lane l holds row lk + 4 r, column 16 qb + lr; S_i sits in column D
    const int sqb = D >> 4, slane = (l & 48) | (D & 15);
    double* P = A.part + (long)s * n * D;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
        const d4 sv = sqb == 0 ? out[ib][0] : (sqb == 1 ? out[ib][1] : out[ib][2]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double S = __shfl(sv[r], slane);
            const int li = w * 32 + ib * 16 + lk + 4 * r;
            const long gi = i0 + li;
#pragma unroll
            for (int qb = 0; qb < LQB; ++qb) {
                const int q = 16 * qb + lr;
                if (q < D && gi < n) P[gi * D + q] = fma(xI[q * LXS + li] - cq[qb], S, -out[ib][qb][r]);
            }
        }
    }
    double* tp = A.tpart + ((long)blockIdx.x * A.S + s) * 4;
    grad_put(tp, 0, t, a_var);
    grad_put(tp, 1, t, a_iso);
    grad_put(tp, 2, t, a_pow);
}

// part[0][i][q] <- 2 sum_s part[s][i][q] in strip order (the dX-sum), dX[i][q] (+)= il_q times it
__global__ void k_latent_sum(double* __restrict__ part, int S, long n, int D, const double* __restrict__ il, double* __restrict__ dX,
                             int accumulate) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * D) return;
    double g = 0.0;
    for (int s = 0; s < S; ++s) g += part[(long)s * n * D + idx];
    g *= 2.0;
    part[idx] = g;
    const double v = il[idx % D] * g;
    dX[idx] = accumulate ? dX[idx] + v : v;
}

// block 0: the theta sums of the nwg workgroups in order; block 1 + q (ARD): rec[2 + q] = sum_i (x~_iq - x~_0q) gs[i][q]
__global__ __launch_bounds__(256) void k_latent_rec(const double* __restrict__ tpart, int nwg, const double* __restrict__ gs,
                                                    const double* __restrict__ Xt, long ldx, long n, int D, int ard, int second,
                                                    double* __restrict__ rec, double* __restrict__ rec2) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int g = t; g < nwg; g += 256)
            for (int c = 0; c < 3; ++c) v[c] += tpart[(long)g * 4 + c];
        grad_put(rec, 0, t, v[0]);
        if (!ard) grad_put(rec, 1, t, v[1]);
        if (second) grad_put(rec2, 0, t, v[2]);
        return;
    }
    const int q = blockIdx.x - 1;
    const double c = Xt[(long)q * ldx];
    double v = 0.0;
    for (long i = t; i < n; i += 256) v = fma(Xt[(long)q * ldx + i] - c, gs[i * D + q], v);
    grad_put(rec, 2 + q, t, v);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static int latent_strips(int nt, int ntj) {            // strips of column steps that fill 256 CUs with nt row blocks
    const int S = (256 + nt - 1) / nt;
    return S > ntj ? ntj : S;
}
size_t latent_part_doubles(long n, int D) {
    const int nt = (int)((n + LT - 1) / LT), ntj = (int)((n + LTJ - 1) / LTJ);
    return (size_t)latent_strips(nt, ntj) * n * D;
}
size_t latent_tpart_doubles(long n) {
    const int nt = (int)((n + LT - 1) / LT), ntj = (int)((n + LTJ - 1) / LTJ);
    return (size_t)nt * latent_strips(nt, ntj) * 4;
}

template <int KIND>
static int launch_k_latent(hipStream_t st, const LatentArgs& A) {
    // the large-LDS opt-in (per device: asked for at every launch, a host call of microseconds)
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_latent_grad<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)LATENT_LDS));
    hipLaunchKernelGGL((k_latent_grad<KIND>), dim3((unsigned)A.nt, (unsigned)A.S), dim3(256), LATENT_LDS, st, A);
    return 0;
}

int launch_latent_grad(hipStream_t st, KernParams kp, const double* Xt, long ldx, long n, const double* W, long ldw,
                       const double* alpha, int Dy, const double* il, double* part, double* tpart, double* dX, int accumulate,
                       double* rec, double* rec2) {
    const int nt = (int)((n + LT - 1) / LT), ntj = (int)((n + LTJ - 1) / LTJ), S = latent_strips(nt, ntj), D = kp.D;
    const LatentArgs A{kp, Xt, ldx, n, W, ldw, alpha, Dy, nt, ntj, S, part, tpart};
    int rc;
    switch (kp.kind) {
    case MI355GP_RBF: rc = launch_k_latent<MI355GP_RBF>(st, A); break;
    case MI355GP_MATERN52: rc = launch_k_latent<MI355GP_MATERN52>(st, A); break;
    case MI355GP_MATERN32: rc = launch_k_latent<MI355GP_MATERN32>(st, A); break;
    case MI355GP_EXPONENTIAL: rc = launch_k_latent<MI355GP_EXPONENTIAL>(st, A); break;
    case MI355GP_RATQUAD: rc = launch_k_latent<MI355GP_RATQUAD>(st, A); break;
    default: mi355gp_set_error("the latent-input gradient pass has no kernel for a %s part", kind_name(kp.kind)); return -1;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_latent_sum, dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, st, part, S, n, D, il, dX, accumulate);
    hipLaunchKernelGGL(k_latent_rec, dim3((unsigned)(1 + (kp.ard ? D : 0))), dim3(256), 0, st, tpart, nt * S, part, Xt, ldx, n, D,
                       kp.ard, kp.kind == MI355GP_RATQUAD ? 1 : 0, rec, rec2);
    return 0;
}

// what the latent entry takes, judged on the host before any device work
int latent_check_parts(int nparts, const mi355gp_part* parts, int D, const char* where) {
    ARG_CHECK(nparts >= 1 && nparts <= 16 && parts, "between 1 and 16 kernel parts");
    if (D > LQ) PART_FAIL("%s: %d latent dimensions: the latent-input gradient pass takes at most %d", where, D, LQ);
    for (int p = 0; p < nparts; ++p) {
        if (!kind_in(parts[p].kind, KS_STATIONARY | KS_STATIC | 1u << MI355GP_RATQUAD))
            PART_FAIL("%s: a %s part has no latent-input gradient pass (RBF, Matern52, Matern32, Exponential, RatQuad, White and Bias have)",
                      where, kind_name(parts[p].kind));
        for (int o = 0; o < p; ++o)
            if (parts[p].term != 0 && parts[o].term == parts[p].term)
                PART_FAIL("%s: product terms (Prod) have no latent-input gradient pass", where);
    }
    return 0;
}

extern "C" {

int mi355gp_latent_set_X(mi355gp_ctx* c, const double* X) {
    ARG_CHECK(c && c->n > 0 && X, "mi355gp_latent_set_X: set_data first");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    HIP_CHECK(hipStreamSynchronize(c->st));
    HIP_CHECK(hipMemcpy(c->dX, X, sizeof(double) * c->n * c->D, hipMemcpyHostToDevice));
    c->hIdxCol = -1;
    return 0;
}

int mi355gp_dbg_latent_grad(int device, int kind, int ard, const double* theta, const double* X, int64_t N, int D, const double* W,
                            const double* alpha, int Dy, double* dX_out, double* rec_out) {
    ARG_CHECK(theta && X && W && alpha && dX_out && rec_out && N > 0 && D > 0 && Dy > 0, "mi355gp_dbg_latent_grad: bad arguments");
    const mi355gp_part in{kind, ard, 0, nullptr, theta, 0};
    if (int rc = latent_check_parts(1, &in, D, "mi355gp_dbg_latent_grad")) return rc;
    if (kind_in(kind, KS_STATIC)) PART_FAIL("mi355gp_dbg_latent_grad: a %s part does not depend on the inputs", kind_name(kind));
    HIP_CHECK(hipSetDevice(device));
    DevicePart pt;
    if (int rc = parse_part(in, D, KS_STATIONARY | 1u << MI355GP_RATQUAD, "mi355gp_dbg_latent_grad", &pt)) return rc;
    if (int rc = pt.upload(0)) return rc;
    const long n = N, np = round_up(N, NB);
    DevBuf dX, dXt, dW, dA, dPart, dT, dOut, dRec;
    HIP_CHECK(dX.alloc(n * D));
    HIP_CHECK(dXt.alloc(D * np));
    HIP_CHECK(dW.alloc(np * np));
    HIP_CHECK(dA.alloc(n * Dy));
    HIP_CHECK(dPart.alloc(latent_part_doubles(n, D)));
    HIP_CHECK(dT.alloc(latent_tpart_doubles(n)));
    HIP_CHECK(dOut.alloc(n * D));
    HIP_CHECK(dRec.alloc(2 * GP_STRIDE));
    HIP_CHECK(hipMemcpy(dX, X, sizeof(double) * n * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dA, alpha, sizeof(double) * n * Dy, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dW, 0, sizeof(double) * np * np));
    HIP_CHECK(hipMemset(dRec, 0, sizeof(double) * 2 * GP_STRIDE));
    HIP_CHECK(hipMemcpy2D(dW, sizeof(double) * np, W, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice));
    launch_scale_inputs(0, dX, n, D, pt.dIl, 1, dXt, np);
    if (int rc = launch_latent_grad(0, pt.kp, dXt, np, n, dW, np, dA, Dy, pt.dIl, dPart, dT, dOut, 0, dRec, dRec + GP_STRIDE)) return rc;
    HIP_CHECK(hipMemcpy(dX_out, dOut, sizeof(double) * n * D, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(rec_out, dRec, sizeof(double) * 2 * GP_STRIDE, hipMemcpyDeviceToHost));
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
