// kern_families.hip -- the covariance kinds that are no function of a distance, each a K-build kernel and a gradient kernel
// around the skeleton of kern_tile.h: Coregionalize, Linear, dot (MLP, Poly).  Each family ends in the two launchers that
// kern.hip's dispatch calls (declared in kern_tile.h); the kernel templates are visible here alone.  (The ext family: kern_ext.hip.)
#include <cstdint>
#include <cstdlib>

#include "../../include/mi355gp.h"
#include "internal.h"
#include "kern_tile.h"

// ------------------------------------------------------------------------------------------------
// Coregionalize (kind 8, coregionalize.py:82-157): k(x, x') = B[idx][idx'], idx = the value of input row kp.col of Xt (staged
// unscaled), B = kp.pw (P x P row-major, P = kp.ard <= 16).  The host validates every index before a launch; an index that is
// not an integer in [0, P) still never reads outside B here: it yields NaN (K-build) or poisons the block's record (gradient).
// (COREG_PMAX and the index guard coreg_idx: internal.h)

// Covariance assembly: the skeleton's tile decode and row epilogue around a lookup -- nothing to accumulate.  B lives in LDS
// once per block, the tile's row / column indices as integers.  The diagonal is what B gives.
template <bool SYM>
__global__ __launch_bounds__(256) void k_kbuild_coreg(KbuildArgs A) {
    __shared__ double sB[COREG_PMAX * COREG_PMAX];
    __shared__ int sa[KT], sb[KT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    const int P = A.kp.ard;
    for (int k = t; k < P * P; k += 256) sB[k] = A.kp.pw[k];
    if (t < KT) {
        const long i = i0 + t;
        sa[t] = (i < A.n) ? coreg_idx(A.Xt1[(long)A.kp.col * A.ld1 + i], P) : 0;
    } else if (t < 2 * KT) {
        const long j = j0 + (t - KT);
        sb[t - KT] = (j < A.m) ? coreg_idx(A.Xt2[(long)A.kp.col * A.ld2 + j], P) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        const int ia = sa[ty * 4 + a];
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            const int jb = sb[tx * 4 + b];
            if (i < A.n && j < A.m) v[b] = (ia >= 0 && jb >= 0) ? sB[ia * P + jb] : __builtin_nan("");
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// The bucketed gradient (see internal.h).  Per tile: the row / column indices go to LDS and two waves OR them into the masks of
// the outputs present among the tile's rows and columns; then, for every present pair (a, b) in a fixed order, each thread sums
// its masked 4 x 4 register elements and a fixed-order wave / block tree reduces them into the block's LDS record.  Rows sorted
// by output (build_XY) give one pair in nearly every tile: one reduction per tile.  FUSED runs over the lower tiles; the second
// sum d (diagonal elements, diagonal tiles only) lets S[b][a] receive the strict lower part once more: the symmetric completion.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_grad_coreg(GradArgs A) {
    __shared__ double sacc[COREG_PMAX * COREG_PMAX];
    __shared__ int sa[KT], sb[KT];
    __shared__ unsigned smask[2];
    __shared__ double red[4][2];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, wv = t >> 6;
    const int P = A.kp.ard;
    for (int k = t; k < P * P; k += 256) sacc[k] = 0.0;
    const double sc = grad_aa_scale<FUSED>(A.aa_scale);
    bool poisoned = false;                                 // (thread 0) an index outside [0, P) was met

    for (long tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, A.ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        __syncthreads();                                   // the previous tile's reads of sa / sb / smask are done
        if (wv < 2) {
            const long r = (wv == 0 ? i0 : j0) + lane;
            int v = -2;                                    // -2: padding (no element), -1: an invalid index
            if (wv == 0 && r < A.n) v = coreg_idx(A.Xt1[(long)A.kp.col * A.ld1 + r], P);
            if (wv == 1 && r < A.m) v = coreg_idx(A.Xt2[(long)A.kp.col * A.ld2 + r], P);
            unsigned bit = (v >= 0) ? (1u << v) : (v == -1 ? (1u << COREG_PMAX) : 0u);
            for (int off = 32; off > 0; off >>= 1) bit |= (unsigned)__shfl_xor((int)bit, off);
            if (wv == 0) sa[lane] = v;
            else sb[lane] = v;
            if (lane == 0) smask[wv] = bit;
        }
        double w[4][4];   // no doubling below the diagonal: sd completes symmetrically
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) w[a][b] = grad_weight<FUSED, false>(A, i0 + ty * 4 + a, j0 + tx * 4 + b, sc);
        __syncthreads();
        const unsigned rm = smask[0], cm = smask[1];
        if (t == 0 && ((rm | cm) >> COREG_PMAX)) poisoned = true;
        int ra[4], cb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) ra[a] = sa[ty * 4 + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) cb[b] = sb[tx * 4 + b];
        const bool diag_tile = FUSED && ti == tj;
        for (unsigned rmm = rm & ((1u << COREG_PMAX) - 1); rmm; rmm &= rmm - 1) {
            const int pa = __ffs(rmm) - 1;
            for (unsigned cmm = cm & ((1u << COREG_PMAX) - 1); cmm; cmm &= cmm - 1) {
                const int pb = __ffs(cmm) - 1;
                double v = 0.0, dg = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (ra[a] == pa && cb[b] == pb) {
                            v += w[a][b];
                            if (diag_tile && ty * 4 + a == tx * 4 + b) dg += w[a][b];
                        }
                for (int off = 32; off > 0; off >>= 1) {
                    v += __shfl_down(v, off);
                    dg += __shfl_down(dg, off);
                }
                if (lane == 0) {
                    red[wv][0] = v;
                    red[wv][1] = dg;
                }
                __syncthreads();
                if (t == 0) {
                    const double sv = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
                    const double sd = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
                    sacc[pa * P + pb] += sv;
                    if (FUSED) sacc[pb * P + pa] += sv - sd;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (t == 0 && poisoned) sacc[0] = __builtin_nan("");
    __syncthreads();
    double* out = A.partials + (long)blockIdx.x * P * P;
    for (int k = t; k < P * P; k += 256) out[k] = sacc[k];
}

int launch_grad_coreg(hipStream_t st, bool fused, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                      long m, const double* G, long ldg, const double* alpha, int Dy, double* partials, const double* aa_scale,
                      const double* Mul, long ldm) {
    const long ntr = (n + KT - 1) / KT, ntc = (m + KT - 1) / KT;
    const long ntiles = fused ? ntr * (ntr + 1) / 2 : ntr * ntc;
    const int nb = pick_grad_blocks(ntiles);
    const GradArgs A = fused ? GradArgs{kp, Xt1, ld1, n, Xt1, ld1, n, G, ldg, alpha, Dy, ntiles, (int)ntr, partials, nullptr, 0, aa_scale,
                                        Mul, ldm, 0}
                             : GradArgs{kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, nullptr, 0, ntiles, (int)ntc, partials, nullptr, 0, nullptr,
                                        nullptr, 0, 0};
    launch_grad_kernel(st, fused, nb, A, k_grad_coreg<true>, k_grad_coreg<false>);
    return nb;
}

// out[j] = kd[j] - sum_i M[i][j]^2: k_col_reduce's variance form with a per-point Kdiag (Coregionalize parts)
__global__ __launch_bounds__(256) void k_col_reduce_vec(const double* __restrict__ M, long ld, long rows, long cols,
                                                        const double* __restrict__ kd, double* __restrict__ out) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + tx;
    double s = 0.0;
    if (j < cols) {
        for (long i = g; i < rows; i += 4) {
            const double x = M[i * ld + j];
            s = fma(x, x, s);
        }
    }
    red[g][tx] = s;
    __syncthreads();
    if (g == 0 && j < cols) out[j] = kd[j] - ((red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]));
}

void launch_col_reduce_vec(hipStream_t st, const double* M, long ld, long rows, long cols, const double* kd, double* out) {
    hipLaunchKernelGGL(k_col_reduce_vec, dim3((unsigned)((cols + 63) / 64)), dim3(256), 0, st, M, ld, rows, cols, kd, out);
}

void launch_kbuild_coreg(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A) {
    const dim3 g((unsigned)nblocks), b(256);
    if (sym) hipLaunchKernelGGL((k_kbuild_coreg<true>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_kbuild_coreg<false>), g, b, 0, st, A);
}

// ------------------------------------------------------------------------------------------------
// Linear (kind 9, linear.py:13-114): K = sum_q var_q x_iq x_jq.  Inputs arrive scaled by sqrt(var_q) on the active dimensions
// (0 elsewhere), so K = sum_q x~_iq x~_jq with no further factor.  Its own kernels around the shared skeleton: the dot product is
// the accumulate step, the sum is the element.  The sum over q runs in the same order for (i, j) and (j, i) and
// fma(a, b, c) = fma(b, a, c): K(X, X) is bitwise symmetric.  The diagonal is what the sum gives (it depends on the point; there
// is no variance to put there).

// s[a][b] += sum_q xi[q][ty*4+a] * xj[q][tx*4+b]
__device__ __forceinline__ void accum_dot(const double* si, const double* sj, int qc, int ty, int tx, double (&s)[4][4]) {
    for (int q = 0; q < qc; ++q) {
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) s[a][b] = fma(xi[a], xj[b], s[a][b]);
    }
}

// Covariance assembly: the element is the sum itself.
template <bool SYM>
__global__ __launch_bounds__(256) void k_kbuild_lin(KbuildArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double s[4][4];
    zero_tile(s);
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC)
            accum_dot(si, sj, stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t), ty, tx, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) v[b] = s[a][b];
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient pass of k_grad for the kind, one launch per group of 32 dimensions (q_off; one launch if !ard).  Record [GP_STRIDE]
// per block: [0] sum g K, ARD [2 + q] sum g x~_iq x~_jq (the host divides by variance / variance_q, linear.py:87-98).
// FUSED: g = 0.5 (sc alpha alpha^T - Dy W) over the lower triangle, off-diagonal weights doubled; else g = G (n x m).
// g is multiplied by Mul (product terms) and, if Hout is given (generic form), written there: the weights of gradients_X.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_grad_lin(GradArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double a_var = 0.0;
    double a_q[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a_q[q] = 0.0;
    const int qcnt = grad_qcnt(A.kp.ard, A.kp.D, A.q_off);
    const double sc = grad_aa_scale<FUSED>(A.aa_scale);

    for (long tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, A.ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double s[4][4];
        zero_tile(s);
        int last_q0 = -1;
        for (int q0 = 0; q0 < A.kp.D; last_q0 = q0, q0 += KDC)
            accum_dot(si, sj, stage_chunk(A, q0, i0, j0, si, sj, t), ty, tx, s);
        double gw[4][4];   // g
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                const double g = grad_weight<FUSED, true>(A, i, j, sc);
                if (!FUSED && A.Hout) store_h<false>(A.Hout, A.ldh, i, j, A.n, A.m, g, g);
                a_var = fma(g, s[a][b], a_var);
                gw[a][b] = g;
            }
        }
        if (qcnt > 0) {
            restage(A, last_q0, qcnt, i0, j0, si, sj, t);
            for_each_dim(si, sj, qcnt, ty, tx, [&](int q, const d4 xi, const d4 xj) {
                double s1 = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    double r = 0.0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) r = fma(gw[a][b], xj[b], r);
                    s1 = fma(xi[a], r, s1);
                }
                a_q[q] += s1;
            });
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]
    double* out = A.partials + (long)blockIdx.x * GP_STRIDE;
    grad_put(out, 0, t, a_var);
    grad_put_dims(out, qcnt, t, a_q);
}

void launch_grad_lin(hipStream_t st, bool fused, const GradArgs& A) {
    const int nb = pick_grad_blocks(A.ntiles);
    for_each_group(A.kp.ard != 0, nb, A,
                   [&](const GradArgs& g) { launch_grad_kernel(st, fused, nb, g, k_grad_lin<true>, k_grad_lin<false>); });
}

void launch_kbuild_lin(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A) {
    const dim3 g((unsigned)nblocks), b(256);
    if (sym) hipLaunchKernelGGL((k_kbuild_lin<true>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_kbuild_lin<false>), g, b, 0, st, A);
}

// ------------------------------------------------------------------------------------------------
// MLP (kind 10, mlp.py:48-147) and Poly (kind 11, poly.py:15-49): functions of the three numbers x.x', x.x and x'.x' of a pair.
// Inputs arrive scaled by sqrt(weight_variance_q) (MLP) / sqrt(scale) (Poly) on the active dimensions, 0 elsewhere, so with
// d_ij = sum_q x~_iq x~_jq, n_i = sum_q x~_iq^2 (both from the same staged slabs, kp.bias = b resp. c0):
//   MLP   s = d + b, p_i = n_i + b:  K = var (2/pi) asin(s / sqrt((p_i + 1)(p_j + 1)))
//   Poly  A = d + c0:                K = var A^order (kp.power; C pow for a negative A)
// Their own kernels around the shared skeleton: dot products (and MLP's norms) accumulate.  The sums over q run in the same
// order for (i, j) and (j, i), fma(a, b, c) = fma(b, a, c) and (p_i + 1)(p_j + 1) commutes: K(X, X) is bitwise symmetric.  n_i is
// the same fma chain as d_ii, so at i == j the element is the formula at s = p_i: var (2/pi) asin(p / sqrt((p + 1)^2)) = Kdiag.

// ni[a] += sum_q xi[q][ty*4+a]^2, nj[b] += sum_q xj[q][tx*4+b]^2
__device__ __forceinline__ void accum_norms(const double* si, const double* sj, int qc, int ty, int tx, double (&ni)[4],
                                            double (&nj)[4]) {
    for (int q = 0; q < qc; ++q) {
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            ni[a] = fma(xi[a], xi[a], ni[a]);
            nj[a] = fma(xj[a], xj[a], nj[a]);
        }
    }
}

#define TWO_OVER_PI 0.63661977236758134308
// the asin argument is below 1 in exact arithmetic (Cauchy-Schwarz on (x~, sqrt b)); the clamp only absorbs a last-bit excess
__device__ __forceinline__ double mlp_k(double var, double s, double qi, double qj) {
    const double t = s / sqrt(qi * qj);
    return var * TWO_OVER_PI * asin(fmin(fmax(t, -1.0), 1.0));
}

// Covariance assembly: the dot products, for MLP the squared norms of both sides as well.
template <bool SYM, int KIND>
__global__ __launch_bounds__(256) void k_kbuild_dot(KbuildArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double s[4][4], ni[4], nj[4];
    zero_tile(s);
#pragma unroll
    for (int a = 0; a < 4; ++a) ni[a] = nj[a] = 0.0;
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC) {
            const int qc = stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t);
            accum_dot(si, sj, qc, ty, tx, s);
            if (KIND == MI355GP_MLP) accum_norms(si, sj, qc, ty, tx, ni, nj);
        }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) {
                const double sb = s[a][b] + A.kp.bias;
                if (KIND == MI355GP_MLP) v[b] = mlp_k(A.kp.variance, sb, ni[a] + A.kp.bias + 1.0, nj[b] + A.kp.bias + 1.0);
                else v[b] = A.kp.variance * pow(sb, A.kp.power);
            } else {
                v[b] = kbuild_pad<SYM>(A, i, j);
            }
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient pass of k_grad for the two kinds, one launch per group of 32 dimensions (q_off; one launch unless MLP with ard).
// Record [GP_STRIDE] per block, g = the weight of the element (below):
//   MLP   c = var (2/pi) g / sqrt((p_i + 1)(p_j + 1) - s^2)                                                  (mlp.py:105)
//         [0] sum g K        [1] sum c (1 - s (1/(p_i+1) + 1/(p_j+1)) / 2)  = d/d bias_variance              (:122)
//         ARD  [2 + q] sum c (x~_iq x~_jq - s (x~_iq^2/(p_i+1) + x~_jq^2/(p_j+1)) / 2)  = w_q d/dw_q           (:107-120)
//         else [2]     sum c (d_ij - s (n_i/(p_i+1) + n_j/(p_j+1)) / 2)                 = w d/dw              (:121)
//   Poly  h = g var order A^(order-1):  [0] sum g K   [1] sum h = d/d bias   [2] sum h d_ij = scale d/d scale (poly.py:36-42)
// FUSED: g = 0.5 (sc alpha alpha^T - Dy W) over the lower triangle, off-diagonal weights doubled (every summand above is
// symmetric in (i, j) when both sides are the same points); else g = G (n x m).  g is multiplied by Mul (product terms).
// Generic form with Hout: c (MLP) is written there -- the weights of gradients_X (mlp.py:124-130, gradx_mlp in parts.h).
// Every sum runs in a fixed order: two evaluations give identical bits.
template <bool FUSED, int KIND>
__global__ __launch_bounds__(256) void k_grad_dot(GradArgs A) {
    constexpr bool MLP = KIND == MI355GP_MLP;
    const KernParams& kp = A.kp;
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double a_var = 0.0, a_b = 0.0, a_w = 0.0;
    double a_q[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a_q[q] = 0.0;
    const int qcnt = grad_qcnt(MLP && kp.ard, kp.D, A.q_off);
    const double sc = grad_aa_scale<FUSED>(A.aa_scale);
    const double coef = MLP ? kp.variance * TWO_OVER_PI : kp.variance * kp.power;

    for (long tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, A.ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double s[4][4], ni[4], nj[4];
        zero_tile(s);
#pragma unroll
        for (int a = 0; a < 4; ++a) ni[a] = nj[a] = 0.0;
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC) {
            const int qc = stage_chunk(A, q0, i0, j0, si, sj, t);
            accum_dot(si, sj, qc, ty, tx, s);
            if (MLP) accum_norms(si, sj, qc, ty, tx, ni, nj);
        }
        // MLP: qi = p_i + 1, hi = 1 / (2 (p_i + 1)); padded rows have x~ = 0, so every quantity below stays finite there
        double qi[4], qj[4], hi[4], hj[4];
        if (MLP) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                qi[a] = ni[a] + kp.bias + 1.0;
                qj[a] = nj[a] + kp.bias + 1.0;
                hi[a] = 0.5 / qi[a];
                hj[a] = 0.5 / qj[a];
            }
        }
        double cw[4][4];            // MLP: c
        double rsum[4], csum[4];    // MLP with ard: row / column sums of c s over this thread's 4 x 4 elements
#pragma unroll
        for (int a = 0; a < 4; ++a) rsum[a] = csum[a] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                const double g = grad_weight<FUSED, true>(A, i, j, sc);
                const double sb = s[a][b] + kp.bias;
                if (MLP) {
                    const double prod = qi[a] * qj[b];
                    const double c = coef * g / sqrt(fma(-sb, sb, prod));
                    const double cs = c * sb;
                    a_var = fma(g, mlp_k(kp.variance, sb, qi[a], qj[b]), a_var);
                    a_b += fma(-cs, hi[a] + hj[b], c);
                    if (qcnt > 0) {
                        rsum[a] += cs;
                        csum[b] += cs;
                    } else {
                        a_w += fma(-cs, ni[a] * hi[a] + nj[b] * hj[b], c * s[a][b]);
                    }
                    cw[a][b] = c;
                    if (!FUSED && A.Hout) store_h<false>(A.Hout, A.ldh, i, j, A.n, A.m, c, c);
                } else {
                    const double pm1 = (i < A.n && j < A.m) ? pow(sb, kp.power - 1.0) : 0.0;
                    const double h = coef * g * pm1;
                    a_var = fma(g, kp.variance * pm1 * sb, a_var);
                    a_b += h;
                    a_w = fma(h, s[a][b], a_w);
                }
            }
        }
        if (MLP && qcnt > 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                rsum[a] *= hi[a];
                csum[a] *= hj[a];
            }
            restage(A, last_q0, qcnt, i0, j0, si, sj, t);
            for_each_dim(si, sj, qcnt, ty, tx, [&](int q, const d4 xi, const d4 xj) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    double r = 0.0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) r = fma(cw[a][b], xj[b], r);
                    s1 = fma(xi[a], r, s1);
                    s2 = fma(rsum[a], xi[a] * xi[a], s2);
                    s2 = fma(csum[a], xj[a] * xj[a], s2);
                }
                a_q[q] += s1 - s2;
            });
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]
    double* out = A.partials + (long)blockIdx.x * GP_STRIDE;
    grad_put(out, 0, t, a_var);
    grad_put(out, 1, t, a_b);
    if (qcnt == 0) grad_put(out, 2, t, a_w);
    grad_put_dims(out, qcnt, t, a_q);
}

template <int KIND>
static void grad_dot(hipStream_t st, bool fused, int nb, const GradArgs& A) {
    launch_grad_kernel(st, fused, nb, A, k_grad_dot<true, KIND>, k_grad_dot<false, KIND>);
}
void launch_grad_dot(hipStream_t st, bool fused, const GradArgs& A) {
    const int nb = pick_grad_blocks(A.ntiles);
    const bool mlp = A.kp.kind == MI355GP_MLP;
    for_each_group(mlp && A.kp.ard, nb, A, [&](const GradArgs& g) {
        if (mlp) grad_dot<MI355GP_MLP>(st, fused, nb, g);
        else grad_dot<MI355GP_POLY>(st, fused, nb, g);
    });
}

template <bool SYM>
static void kbuild_dot(hipStream_t st, long nblocks, const KbuildArgs& A) {
    const dim3 g((unsigned)nblocks), b(256);
    switch (A.kp.kind) {
    case MI355GP_MLP: hipLaunchKernelGGL((k_kbuild_dot<SYM, MI355GP_MLP>), g, b, 0, st, A); break;
    default: hipLaunchKernelGGL((k_kbuild_dot<SYM, MI355GP_POLY>), g, b, 0, st, A); break;
    }
}
void launch_kbuild_dot(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A) {
    if (sym) kbuild_dot<true>(st, nblocks, A);
    else kbuild_dot<false>(st, nblocks, A);
}
