// kern.hip -- the stationary kinds' covariance assembly (Stationary.K) and fused dL/dK -> dL/dtheta reduction
// (Stationary.update_gradients_full), and the dispatch of both stages over every kind.
// Reference: GPy/kern/src/stationary.py:105-168,193-243; rbf.py:51-52,177-178; stationary.py:382-386,
// 488-492,585-589; stationary_cython.pyx:53-62; inference/.../exact_gaussian_inference.py:55-72.
//
// These stages are HBM-bound (8 N^2 bytes written by the build, 4 N^2 read by the gradient pass over the
// lower triangle of Ky^-1): inputs are pre-scaled by 1/lengthscale and stored dimension-major so a 64-point
// slab of every dimension is one coalesced 512-byte read, X tiles live in LDS, and K is recomputed from X
// inside the gradient pass instead of being re-read from memory.
// The pieces every kind's kernels share are in kern_tile.h; the other kinds' kernels in kern_families.hip, the streaming
// sparse path's in kern_sparse.hip, the reductions and fetch helpers that stage no input slabs in reduce.hip.
#include <cstdint>
#include <cstdlib>

#include "../../include/mi355gp.h"
#include "grad_policy.h"
#include "internal.h"
#include "kern_tile.h"

// ------------------------------------------------------------------------------------------------
// Xt[q][i] = X[i][q] / l_q, zero for i in [n, ldx)
__global__ void k_scale_inputs(const double* __restrict__ X, long n, int D, const double* __restrict__ inv_ls,
                               int ard, double* __restrict__ Xt, long ldx) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)D * ldx) return;
    const int q = (int)(idx / ldx);
    const long i = idx - (long)q * ldx;
    Xt[idx] = (i < n) ? X[i * D + q] * inv_ls[ard ? q : 0] : 0.0;
}

void launch_scale_inputs(hipStream_t st, const double* X, long n, int D, const double* inv_ls, int ard,
                         double* Xt, long ldx) {
    const long total = (long)D * ldx;
    hipLaunchKernelGGL(k_scale_inputs, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, n, D, inv_ls,
                       ard, Xt, ldx);
}

// The stationary kinds and the static ones.  White puts its variance on coinciding points: the diagonal of a symmetric
// build, and of a rectangular one that says so (diag_same).  The one kernel that takes KbuildArgs' fields as parameters of
// its own: `__restrict__` on them is worth a wait less in the epilogue of the kernel that the benchmark times.
template <bool SYM>
__global__ __launch_bounds__(256) void k_kbuild(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                const double* __restrict__ Xt2, long ld2, long m,
                                                double* __restrict__ out, long ldo, long nrows_out,
                                                const double* __restrict__ noise, long noise_len, double jit,
                                                int lower_only, int add_diag, int ntc, int accumulate, int diag_same,
                                                const double* mul) {
    const KbuildArgs A{kp,    Xt1,        ld1,      n,   Xt2,        ld2,       m,  out, ldo, nrows_out, noise, noise_len,
                       jit,   lower_only, add_diag, ntc, accumulate, diag_same, mul};
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double r2[4][4];
    zero_tile(r2);
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC)
            accum_r2(si, sj, stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t), ty, tx, r2);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) v[b] = cov_k(A.kp.kind, A.kp.variance, r2[a][b], (SYM || A.diag_same) && i == j);
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient reduction of the stationary kinds (the records and the shared pieces: kern_tile.h)
template <bool FUSED, bool ARD>
__global__ __launch_bounds__(256) void k_grad(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                              const double* __restrict__ Xt2, long ld2, long m,
                                              const double* __restrict__ G, long ldg,
                                              const double* __restrict__ alpha, int Dy, int q_off,
                                              long ntiles, int ntc, double* __restrict__ partials,
                                              double* __restrict__ Hout = nullptr, long ldh = 0, int diag_same = 0,
                                              const double* __restrict__ aa_scale = nullptr,
                                              const double* __restrict__ Mul = nullptr, long ldm = 0,
                                              RankTerm rk = RankTerm{nullptr, nullptr, 0, 0.0, 1.0, nullptr}) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double a_var = 0.0, a_iso = 0.0;
    double a_q[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a_q[q] = 0.0;
    const int qcnt = grad_qcnt(ARD, kp.D, q_off);
    const double sc = grad_aa_scale<FUSED>(aa_scale);

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double r2[4][4];
        zero_tile(r2);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC)
            accum_r2(si, sj, stage_chunk(kp.D, q0, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t), ty, tx, r2);
        // weights * dL_dK, then the covariance factors
        double gT[4][4];   // g * dK/dr / r
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0;   // grad_weight<FUSED, true> with the rank term, spelt out: see there
                if (i < n && j < m) {
                    if (FUSED) {
                        if (j <= i) {
                            double aa = 0.0;
                            for (int d = 0; d < Dy; ++d) aa = fma(alpha[i * Dy + d], alpha[j * Dy + d], aa);
                            g = 0.5 * (sc * aa - (double)Dy * G[i * ldg + j]);
                            if (j < i) g *= 2.0;
                        }
                    } else {
                        g = G[i * ldg + j];
                        if (rk.Y) {   // dL_dKnm = gscale * G + beta * Y v^T formed on the fly (var_dtc.py:219,233)
                            double yv = 0.0;
                            for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                            g = fma(rk.gscale, g, rk.beta * yv);
                            if (rk.rowscale) g *= rk.rowscale[i];   // per-point precision (var_dtc.py:224-226)
                        }
                    }
                    if (Mul) g *= Mul[i * ldm + j];
                }
                const CovVal c = cov_all(kp.kind, kp.variance, r2[a][b], (FUSED || diag_same) && i == j);
                a_var = fma(g, c.k, a_var);
                if (!ARD) a_iso = fma(g, c.dk_r, a_iso);
                gT[a][b] = g * c.dk_or;
            }
        }
        if (!FUSED && Hout) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) store_h<true>(Hout, ldh, i0 + ty * 4 + a, j0 + tx * 4 + b, n, m, r2[a][b], gT[a][b]);
        }
        if (ARD) {
            restage(last_q0, q_off, qcnt, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t);
#pragma unroll
            for (int q = 0; q < KDC; ++q) {   // (for_each_dim spelt out: through the lambda the ARD instantiations' code moves)
                if (q < qcnt) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    double s = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const double d = xi[a] - xj[b];
                            s = fma(gT[a][b], d * d, s);
                        }
                    a_q[q] += s;
                }
            }
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    grad_put(out, 0, t, a_var);
    if (!ARD) grad_put(out, 1, t, a_iso);
    else grad_put_dims(out, qcnt, t, a_q);
}

// k_grad<true, true> of the plain stationary kinds with less fp64 issue per tile (grad_policy.h says which launches take it).
//   * Interior tiles (strictly below the diagonal, all 64 rows inside n) need no bounds or triangle test: alpha is read once per
//     thread row and column, the weights of a thread row are ONE 32-byte load, every element counts twice.  Diagonal and edge tiles
//     form their weights as k_grad does.
//   * r^2, K and the variance sum keep k_grad's direct form (x~_i - x~_j)^2: exact zeros for duplicates.
//   * The per-dimension reduction  a_q += sum_ij T_ij (x~_iq - x~_jq)^2,  T = g (dK/dr)/r  (48 fp64 instructions per thread and
//     dimension as sub + mul + fma per pair), is expanded about a per-tile centre c_q = x~_{j0,q}, u = x~_i - c, v = x~_j - c:
//         sum_i u_iq (u_iq R_i - 2 P_iq) + sum_j v_jq^2 C_j,    R = row sums of T, C = column sums, P = T V  (64 x 64 x qpad)
//     with P on v_mfma_f64_16x16x4: wave w owns rows 16 w .. 16 w + 15 (its four ty), q in blocks of 16, 32 MFMAs per tile and wave
//     at D = 32.  T reaches the A operand through a per-wave LDS scratch, one of the thread's four columns at a time (16 columns:
//     8.5 KB for the block); MFMA row m reads scratch row 4 (m & 3) + (m >> 2), so that accumulator register r of lane (ty, tx) is
//     P[4 ty + r][16 qb + tx]: the thread's OWN rows, and R needs no more than the sum over the 16 lanes of a row group.  The centring
//     is applied as the operands leave LDS (the slabs stay as the r^2 pass needs them: one staging), so u, v are differences of
//     points of ONE tile and the expansion cancels at the tile's spread, not at the data's offset from the origin.
//   * Two accumulators per lane (q = tx, 16 + tx) replace a_q[32]; every sum runs in a fixed order: bit reproducible.
//   * The kind is a template parameter: 167 VGPRs and three waves per SIMD without a spill (254 with the kind at run time).
// Slab row strides 66 / 74 (not 64 / 72): lanes that differ in q (the MFMA's B operand, the u and v reads) fall on different banks.
// LDS: 16.5 + 18.5 + 8.5 + 2 + 2 = 47.5 KB, three blocks per CU.
#define TG_SI 66
#define TG_SJ 74
#define TG_AS 17
__device__ __forceinline__ int tg_stage(int D, int q0, const double* __restrict__ Xt, long ldx, long i0, long j0, double* si,
                                        double* sj, int t) {
    const int qc = (D - q0 < KDC) ? (D - q0) : KDC;
    const int qpad = (qc + 15) & ~15;                    // dimensions up to the next multiple of 16 are zeros: the MFMA's q blocks
    __syncthreads();
    for (int idx = t; idx < qpad * KT; idx += 256) {
        const int q = idx >> 6, ii = idx & 63;
        const bool in = q < qc;
        si[q * TG_SI + ii] = in ? Xt[(long)(q0 + q) * ldx + i0 + ii] : 0.0;
        sj[q * TG_SJ + xj_pos(ii)] = in ? Xt[(long)(q0 + q) * ldx + j0 + ii] : 0.0;
    }
    __syncthreads();
    return qc;
}

template <int KIND>
__global__ __launch_bounds__(256, 3) void k_grad_tilegemm(KernParams kp, const double* __restrict__ Xt, long ldx, long n,
                                                          const double* __restrict__ W, long ldw,
                                                          const double* __restrict__ alpha, int Dy, int q_off, long ntiles,
                                                          double* __restrict__ partials, const double* __restrict__ aa_scale) {
    __shared__ __attribute__((aligned(16))) double si[KDC * TG_SI];
    __shared__ __attribute__((aligned(16))) double sj[KDC * TG_SJ];
    __shared__ double sa[4 * 16 * TG_AS];                 // per wave: 16 rows x 16 columns of T
    __shared__ __attribute__((aligned(16))) double scs[4 * KT];   // per wave: the column sums of its 16 rows
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, w = t >> 6, kk = ty & 3;
    const int qcnt = (kp.D - q_off < KDC) ? (kp.D - q_off) : KDC;
    const bool two = qcnt > 16;                           // a second block of 16 dimensions
    const double sc = aa_scale ? aa_scale[0] : 1.0;
    double* saw = sa + w * 16 * TG_AS;
    const int arow = (4 * (tx & 3) + (tx >> 2)) * TG_AS + kk;
    double a_var = 0.0, acc0 = 0.0, acc1 = 0.0;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<true>(tile, 0, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double r2[4][4];
        zero_tile(r2);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC) {
            const int qc = tg_stage(kp.D, q0, Xt, ldx, i0, j0, si, sj, t);
            for (int q = 0; q < qc; ++q) {
                const d2 xa = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4);
                const d2 xb = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4 + 2);
                const double xi[4] = {xa[0], xa[1], xb[0], xb[1]};
                const d2 lo = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 2 * tx);
                const d2 hi = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 40 + 2 * tx);
                const double xj[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const double d = xi[a] - xj[b];
                        r2[a][b] = fma(d, d, r2[a][b]);
                    }
            }
        }
        // T = g (dK/dr)/r and the variance sum
        double gT[4][4];
        if (tj < ti && i0 + KT <= n) {
            const long ib = i0 + ty * 4, jb = j0 + tx * 4;
            if (Dy == 1) {
                double ai[4], aj[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) ai[a] = alpha[ib + a], aj[a] = alpha[jb + a];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) gT[a][b] = fma(ai[a], aj[b], 0.0);
            } else {
                zero_tile(gT);
                for (int d = 0; d < Dy; ++d) {
                    double ai[4], aj[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) ai[a] = alpha[(ib + a) * Dy + d], aj[a] = alpha[(jb + a) * Dy + d];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) gT[a][b] = fma(ai[a], aj[b], gT[a][b]);
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const d4 wv = *reinterpret_cast<const d4*>(W + (ib + a) * ldw + jb);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    double g = 0.5 * (sc * gT[a][b] - (double)Dy * wv[b]);
                    g *= 2.0;
                    const CovVal c = cov_all(KIND, kp.variance, r2[a][b], false);
                    a_var = fma(g, c.k, a_var);
                    gT[a][b] = g * c.dk_or;
                }
            }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const long i = i0 + ty * 4 + a;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const long j = j0 + tx * 4 + b;
                    double g = 0.0;
                    if (i < n && j <= i) {
                        double aa = 0.0;
                        for (int d = 0; d < Dy; ++d) aa = fma(alpha[i * Dy + d], alpha[j * Dy + d], aa);
                        g = 0.5 * (sc * aa - (double)Dy * W[i * ldw + j]);
                        if (j < i) g *= 2.0;
                    }
                    const CovVal c = cov_all(KIND, kp.variance, r2[a][b], i == j);
                    a_var = fma(g, c.k, a_var);
                    gT[a][b] = g * c.dk_or;
                }
            }
        }
        // bring the dimensions this launch reduces back (D > 32)
        if (last_q0 != q_off) tg_stage(kp.D, q_off, Xt, ldx, i0, j0, si, sj, t);
        // R: over the 16 lanes of the row group; C: over the wave's four row groups here, over the waves below
        double R[4], C[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            R[a] = (gT[a][0] + gT[a][1]) + (gT[a][2] + gT[a][3]);
            C[a] = (gT[0][a] + gT[1][a]) + (gT[2][a] + gT[3][a]);
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
#pragma unroll
            for (int a = 0; a < 4; ++a) R[a] += __shfl_xor(R[a], m);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            C[b] += __shfl_xor(C[b], 16);
            C[b] += __shfl_xor(C[b], 32);
        }
        if (kk == 0) {
            *reinterpret_cast<d2*>(scs + w * KT + 4 * tx) = (d2){C[0], C[1]};
            *reinterpret_cast<d2*>(scs + w * KT + 4 * tx + 2) = (d2){C[2], C[3]};
        }
        // P = T V: column 4 tx' + b of the tile is k index tx' of chunk b
        const double c0 = sj[tx * TG_SJ], c1 = two ? sj[(16 + tx) * TG_SJ] : 0.0;   // the centre: column point 0 (xj_pos(0) = 0)
        d4 P0 = {0.0, 0.0, 0.0, 0.0}, P1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int a = 0; a < 4; ++a) saw[(4 * kk + a) * TG_AS + tx] = gT[a][b];
            __builtin_amdgcn_wave_barrier();
            const double* vb = sj + tx * TG_SJ + 40 * (b >> 1) + (b & 1) + 2 * kk;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double av = saw[arow + 4 * s];
                P0 = mfma_f64(av, vb[8 * s] - c0, P0);
                if (two) P1 = mfma_f64(av, vb[16 * TG_SJ + 8 * s] - c1, P1);
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();                                     // the waves' column sums are there
        // the thread's share: dimensions tx (and 16 + tx), rows 4 ty .. + 3 (its own), columns 4 ty .. + 3
        double Cs[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) Cs[b] = scs[4 * ty + b];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww)
#pragma unroll
            for (int b = 0; b < 4; ++b) Cs[b] += scs[ww * KT + 4 * ty + b];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            if (qb == 0 || two) {
                const int q = 16 * qb + tx;
                const double c = qb ? c1 : c0;
                const d4 P = qb ? P1 : P0;
                const d2 ua = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4);
                const d2 ub = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4 + 2);
                const d2 va = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 2 * ty);
                const d2 vc = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 40 + 2 * ty);
                const double u[4] = {ua[0] - c, ua[1] - c, ub[0] - c, ub[1] - c};
                const double v[4] = {va[0] - c, va[1] - c, vc[0] - c, vc[1] - c};
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) s = fma(u[a], fma(u[a], R[a], -2.0 * P[a]), s);
#pragma unroll
                for (int b = 0; b < 4; ++b) s = fma(v[b] * v[b], Cs[b], s);
                if (qb) acc1 += s;
                else acc0 += s;
            }
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]: dimension 16 qb + tx over the 16 row groups in order
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    double* red = block_red();
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        if (qb == 0 || two) {
            __syncthreads();
            red[t] = qb ? acc1 : acc0;
            __syncthreads();
            if (t < 16 && 16 * qb + t < qcnt) {
                double s = 0.0;
                for (int r = 0; r < 16; ++r) s += red[r * 16 + t];
                out[2 + 16 * qb + t] = s;
            }
        }
    }
}

int grad_num_blocks(long n) {
    const long nt = (n + KT - 1) / KT;
    return pick_grad_blocks(nt * (nt + 1) / 2);
}

int grad_generic_num_blocks(long n, long m) {
    return pick_grad_blocks(((n + KT - 1) / KT) * ((m + KT - 1) / KT));
}

// ------------------------------------------------------------------------------------------------
// The launch functions of the assembly and gradient kernels: each prepares its geometry, one dispatch picks the kind's kernel.
template <bool SYM>
static void launch_kbuild(hipStream_t st, long nblocks, const KbuildArgs& A) {
    switch (A.kp.kind) {
    case MI355GP_RATQUAD:
    case MI355GP_STDPERIODIC:
    case MI355GP_COSINE:
    case MI355GP_SINC:
    case MI355GP_EXPQUADCOSINE: launch_kbuild_ext(st, SYM, nblocks, A); break;
    case MI355GP_COREGIONALIZE: launch_kbuild_coreg(st, SYM, nblocks, A); break;
    case MI355GP_LINEAR: launch_kbuild_lin(st, SYM, nblocks, A); break;
    case MI355GP_MLP:
    case MI355GP_POLY: launch_kbuild_dot(st, SYM, nblocks, A); break;
    default:
        hipLaunchKernelGGL((k_kbuild<SYM>), dim3((unsigned)nblocks), dim3(256), 0, st, A.kp, A.Xt1, A.ld1, A.n, A.Xt2, A.ld2, A.m,
                           A.out, A.ldo, A.nrows_out, A.noise, A.noise_len, A.jit, A.lower_only, A.add_diag, A.ntc, A.accumulate,
                           A.diag_same, A.mul);
        break;
    }
}

void launch_kbuild_sym(hipStream_t st, KernParams kp, const double* Xt, long ldx, long n, long npad, double* A,
                       const double* noise, long noise_len, double jit, int lower_only, int add_diag, int accumulate,
                       const double* mul) {
    const int nt = (int)(npad / KT);
    launch_kbuild<true>(st, (long)nt * nt, KbuildArgs{kp, Xt, ldx, n, Xt, ldx, n, A, npad, npad, noise, noise_len, jit, lower_only,
                                                      add_diag, nt, accumulate, 0, mul});
}

void launch_kbuild_cross(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                         long ld2, long m, double* Kout, long ldk, int accumulate, int diag_same, const double* mul) {
    const int ntr = (int)((n + KT - 1) / KT), ntc = (int)((m + KT - 1) / KT);
    launch_kbuild<false>(st, (long)ntr * ntc, KbuildArgs{kp, Xt1, ld1, n, Xt2, ld2, m, Kout, ldk, n, nullptr, 0, 0.0, 0, 0, ntc,
                                                         accumulate, diag_same, mul});
}

// k_grad and k_grad_tilegemm take GradArgs' fields as parameters of their own, as k_kbuild does (they are what the benchmark
// times): the one place each list is written out besides the kernel's signature
template <bool FUSED, bool ARD>
static void launch_k_grad(hipStream_t st, int nb, const GradArgs& A, int diag_same, RankTerm rk) {
    hipLaunchKernelGGL((k_grad<FUSED, ARD>), dim3((unsigned)nb), dim3(256), 0, st, A.kp, A.Xt1, A.ld1, A.n, A.Xt2, A.ld2, A.m, A.G, A.ldg,
                       A.alpha, A.Dy, A.q_off, A.ntiles, A.ntc, A.partials, A.Hout, A.ldh, diag_same, A.aa_scale, A.Mul, A.ldm, rk);
}
template <int KIND>
static void launch_k_grad_tilegemm(hipStream_t st, int nb, const GradArgs& A) {
    hipLaunchKernelGGL((k_grad_tilegemm<KIND>), dim3((unsigned)nb), dim3(256), 0, st, A.kp, A.Xt1, A.ld1, A.n, A.G, A.ldg, A.alpha, A.Dy,
                       A.q_off, A.ntiles, A.partials, A.aa_scale);
}

// fused: over the lower tiles of W (n x n); else over the ntiles = ntr * ntc tiles of G.  The sparse path's rank term (rk) and
// diag_same are the stationary kernel's alone: that path has no other kind.
static void launch_grad(hipStream_t st, bool fused, const GradArgs& A, int diag_same, RankTerm rk) {
    const KernParams& kp = A.kp;
    if (kp.kind == MI355GP_COREGIONALIZE) return;          // (launch_grad_coreg: records of its own shape)
    if (kp.kind >= MI355GP_RATQUAD) {
        if (rk.Y) return;
        const bool dot = kp.kind == MI355GP_MLP || kp.kind == MI355GP_POLY;
        (dot ? launch_grad_dot : kp.kind == MI355GP_LINEAR ? launch_grad_lin : launch_grad_ext)(st, fused, A);
        return;
    }
    const int nb = pick_grad_blocks(A.ntiles);
    static const int force_old = !diag_env_int(DIAG_ENV("GRAD_TILEGEMM"), 1);   // MI355GP_GRAD_TILEGEMM=0: k_grad everywhere (A/B)
    const bool tilegemm = grad_tilegemm_applies(GradLaunchCase{fused, kp.kind, kp.ard, A.Mul != nullptr, A.Hout != nullptr,
                                                               rk.Y != nullptr, (uintptr_t)A.G, A.ldg, force_old});
    for_each_group(kp.ard != 0, nb, A, [&](const GradArgs& g) {
        if (tilegemm) {
            if (kp.kind == MI355GP_RBF) launch_k_grad_tilegemm<MI355GP_RBF>(st, nb, g);
            else if (kp.kind == MI355GP_MATERN52) launch_k_grad_tilegemm<MI355GP_MATERN52>(st, nb, g);
            else launch_k_grad_tilegemm<MI355GP_MATERN32>(st, nb, g);
        } else if (fused) {
            if (kp.ard) launch_k_grad<true, true>(st, nb, g, diag_same, rk);
            else launch_k_grad<true, false>(st, nb, g, diag_same, rk);
        } else {
            if (kp.ard) launch_k_grad<false, true>(st, nb, g, diag_same, rk);
            else launch_k_grad<false, false>(st, nb, g, diag_same, rk);
        }
    });
}

void launch_grad_fused(hipStream_t st, KernParams kp, const double* Xt, long ldx, long n, const double* W,
                       long ldw, const double* alpha, int Dy, double* partials, const double* aa_scale,
                       const double* Mul, long ldm) {
    const long nt = (n + KT - 1) / KT;
    launch_grad(st, true, GradArgs{kp, Xt, ldx, n, Xt, ldx, n, W, ldw, alpha, Dy, nt * (nt + 1) / 2, (int)nt, partials, nullptr, 0,
                                   aa_scale, Mul, ldm, 0},
                0, RankTerm{nullptr, nullptr, 0, 0.0, 1.0, nullptr});
}

void launch_grad_generic(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                         long ld2, long m, int symmetric, const double* G, long ldg, double* partials,
                         double* Hout, long ldh, RankTerm rk) {
    const long ntr = (n + KT - 1) / KT, ntc = (m + KT - 1) / KT;
    launch_grad(st, false, GradArgs{kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, nullptr, 0, ntr * ntc, (int)ntc, partials, Hout, ldh,
                                    nullptr, nullptr, 0, 0},
                symmetric, rk);
}
